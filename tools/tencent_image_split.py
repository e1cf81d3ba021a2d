#!/usr/bin/env python
"""``TencentImageSplitTool`` of the reference's root ``tencent_image_split.py`` on the device: the traffic-sign recipe's
big pictures cut into overlapping tiles, each tile that holds a sign's centre written as ``<id>_<w_off>_<h_off>.jpg`` with
its ``.circle`` label file.

Per batch of source files ONE decode (``image_io.decode_into``, EXIF orientation applied as ``cv2.imread`` applies it) and
ONE encode (``image_io.encode_into``): a tile is a ``placement`` entry ``(shape, byte offset, source pitch)`` that points
into the decoded picture, so no pixel is copied.  The encoder reads pixels as single bytes, rows by ``src_off + y *
src_pitch`` and columns clamped to the tile's own width (csrc/jpeg_enc_core.h:184-191), and the library checks every entry
against the buffer before the launch (csrc/jpeg_enc_host.cpp:95-99): a tile's offset of ``3 * w_off`` bytes and the
source's pitch need no alignment, so no tile is encoded from a copy.  The files are what ``cv2.imwrite`` writes at its
defaults (quality 95, 4:2:0) for the same crop.

The tile loop is the reference's (tencent_image_split.py:57-95): offsets step by ``tile - overlap``, every offset after
the first is clamped to ``size - tile`` (``min(h - h_s, h_off)``; a second step exists only where the picture is larger
than a tile, so no offset is negative), a picture smaller than a tile gives one short tile, a label goes to every tile
whose inclusive range ``[off, off + tile - 1]`` holds its centre, boxes are ``int(float(text))`` and shifted by the
offsets.  ``num_process`` is accepted and unused (the batch is the device's).  Sources are taken in sorted name order.

    python tools/tencent_image_split.py IN_ROOT OUT_ROOT [--tile 640 640] [--overlap 160 160] [--batch 16]
"""
import argparse
import glob
import os
import os.path as osp
import sys

ROOT = osp.dirname(osp.dirname(osp.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_annotation(lines):
    """tencent_image_split.py:42-55: per row ``dict(bbox=[x, y, w, h] ints, labeltxt=fields 1..3, center)``."""
    objects = []
    for si in lines:
        bbox_info = si.split(',')
        assert len(bbox_info) == 8
        bbox = [int(float(x)) for x in bbox_info[4:]]
        objects.append(dict(bbox=bbox, labeltxt=bbox_info[1:4], center=(bbox[0] + 0.5 * bbox[2], bbox[1] + 0.5 * bbox[3])))
    return objects


def tiles_of(h, w, objs, tile_shape, tile_overlap):
    """tencent_image_split.py:67-95 for an (h, w) picture -> ``[(w_off, h_off, tile height, tile width, label lines)]``
    of the tiles that hold a centre, in the reference's order.  The tile's extent is what the slice
    ``img[h_off:h_off + h_s, w_off:w_off + w_s]`` gives."""
    w_ovr, h_ovr = tile_overlap
    w_s, h_s = tile_shape
    out = []
    for h_off in range(0, max(1, h - h_ovr), h_s - h_ovr):
        if h_off > 0:
            h_off = min(h - h_s, h_off)
        for w_off in range(0, max(1, w - w_ovr), w_s - w_ovr):
            if w_off > 0:
                w_off = min(w - w_s, w_off)
            inside = [o for o in objs if w_off <= o['center'][0] <= w_off + w_s - 1 and h_off <= o['center'][1] <= h_off + h_s - 1]
            if not inside:
                continue
            lines = []
            for row, o in enumerate(inside):
                box = o['bbox'][:]
                box[0] -= w_off
                box[1] -= h_off
                lines.append(f'{row},{",".join(o["labeltxt"])},{",".join(str(v) for v in box)}\n')
            out.append((w_off, h_off, min(h_s, h - h_off), min(w_s, w - w_off), lines))
    return out


class TencentImageSplitTool:

    def __init__(self, in_root, out_root, tile_overlap, tile_shape, num_process=8, batch=16, device=None):
        self.in_images_dir, self.in_labels_dir = osp.join(in_root, 'img/'), osp.join(in_root, 'label/')
        self.out_images_dir, self.out_labels_dir = osp.join(out_root, 'img/'), osp.join(out_root, 'label/')
        assert isinstance(tile_shape, tuple), f'argument "tile_shape" must be tuple but got {type(tile_shape)} instead!'
        assert isinstance(tile_overlap, tuple), f'argument "tile_overlap" must be tuple but got {type(tile_overlap)} instead!'
        self.tile_overlap, self.tile_shape = tile_overlap, tile_shape
        image_ids = [osp.splitext(osp.split(x)[-1])[0] for x in glob.glob(self.in_images_dir + '*.jpg')]
        label_ids = [osp.splitext(osp.split(x)[-1])[0] for x in glob.glob(self.in_labels_dir + '*.circle')]
        assert set(image_ids) == set(label_ids)
        self.image_ids = sorted(image_ids)
        for d in (out_root, self.out_images_dir, self.out_labels_dir):
            os.makedirs(d, exist_ok=True)
        self.num_process, self.batch, self.device = num_process, int(batch), device
        if self.batch < 1:
            raise ValueError(f'batch {batch!r} is not positive')

    def _objects(self, image_id):
        with open(osp.join(self.in_labels_dir, image_id + '.circle'), 'r') as f:
            return parse_annotation(f.readlines())

    def _split_batch(self, ids):
        """One decode and one encode for the source files ``ids`` -> the tile names written."""
        import torch
        from mmdet_yolov4_amd import image_io
        dev = torch.device(self.device) if self.device is not None else torch.device('cuda', torch.cuda.current_device())
        bufs = []
        for i in ids:
            with open(osp.join(self.in_images_dir, i + '.jpg'), 'rb') as f:
                bufs.append(f.read())
        for k, e in image_io.refusals(bufs).items():
            raise NotImplementedError(f'{osp.join(self.in_images_dir, ids[k] + ".jpg")}: {e}')
        pixels, table = image_io.decode_into(bufs, 'bgr', dev, orientation=True)
        placement, names, labels = [], [], []
        for i, t in zip(ids, table):
            h, w = image_io.oriented_size(t)
            off, pitch = int(t.out_off), int(t.out_pitch)
            for w_off, h_off, th, tw, lines in tiles_of(h, w, self._objects(i), self.tile_shape, self.tile_overlap):
                # the tile where it lies in the decoded picture: in bounds by construction (h_off + th <= h, w_off + tw <= w)
                placement.append(((th, tw, 3), off + h_off * pitch + 3 * w_off, pitch))
                names.append(f'{i}_{w_off}_{h_off}')
                labels.append(lines)
        if not placement:
            return []
        files = image_io.encode_into(pixels, placement)
        for name, data, lines in zip(names, files, labels):
            with open(osp.join(self.out_images_dir, name + '.jpg'), 'wb') as f:
                f.write(data)
            with open(osp.join(self.out_labels_dir, name + '.circle'), 'w') as f:
                f.writelines(lines)
        return names

    def split(self):
        written = []
        for k in range(0, len(self.image_ids), self.batch):
            written += self._split_batch(self.image_ids[k:k + self.batch])
        return written


def main(argv=None):
    p = argparse.ArgumentParser(description='cut the pictures of IN_ROOT/img (labels in IN_ROOT/label) into tiles')
    p.add_argument('in_root')
    p.add_argument('out_root')
    p.add_argument('--tile', type=int, nargs=2, default=(640, 640), metavar=('W', 'H'))
    p.add_argument('--overlap', type=int, nargs=2, default=(160, 160), metavar=('W', 'H'))
    p.add_argument('--batch', type=int, default=16, help='source files per decode and encode call')
    args = p.parse_args(argv)
    tool = TencentImageSplitTool(args.in_root, args.out_root, tile_overlap=tuple(args.overlap), tile_shape=tuple(args.tile),
                                 batch=args.batch)
    print(f'{len(tool.split())} tiles from {len(tool.image_ids)} pictures -> {args.out_root}')


if __name__ == '__main__':
    main()
