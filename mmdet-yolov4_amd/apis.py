"""``inference_detector`` under the reference's name (``mmdet/apis/inference.py:88-158``).

The reference composes ``cfg.data.test.pipeline`` per image on the CPU (mmcv / OpenCV), collates, scatters and calls
``model(return_loss=False, rescale=True, **data)``.  Here the same pipeline block drives ``FusedTestPipeline`` (one
launch per image, parity unpinned -- see ``preprocess.py``) and the detector's fused ``simple_test``.  Image files are
read by ``image_io.imread`` (the reference reads them with ``mmcv.imread``): baseline JPEG, decoded on the GPU to the
bytes libjpeg-turbo gives; EXIF orientation is not applied."""
import os

import numpy as np
import torch

from .image_io import imread

from .preprocess import FusedTestPipeline


def inference_detector(model, imgs, test_pipeline=None):
    """``imgs``: an (h, w, 3) uint8 array (BGR, as ``mmcv.imread`` returns), a (h, w, 3) ``torch.uint8`` tensor on the
    model's device, a file name (``str`` / ``os.PathLike``: a baseline JPEG, decoded on the GPU) or a list / tuple of
    them, mixed freely.  Returns the per-image result (a list of per-class (k, 5) arrays) or, for a list, the list of
    them -- like the reference.  ``test_pipeline`` defaults to ``model.cfg.data.test.pipeline``."""
    is_batch = isinstance(imgs, (list, tuple))
    if not is_batch:
        imgs = [imgs]
    for i in imgs:
        if not isinstance(i, (np.ndarray, torch.Tensor, str, os.PathLike)):
            raise TypeError(f'inference_detector takes arrays, uint8 tensors and file names, not {type(i).__name__}')
    if test_pipeline is None:
        cfg = getattr(model, 'cfg', None)
        if cfg is None:
            raise ValueError('pass test_pipeline= or attach the config as model.cfg (init_detector does in the reference)')
        test_pipeline = cfg.data.test.pipeline
    device = next(model.parameters()).device
    pipe = test_pipeline if callable(test_pipeline) else FusedTestPipeline.from_config(test_pipeline, device=device)
    imgs = list(imgs)
    files = [k for k, i in enumerate(imgs) if isinstance(i, (str, os.PathLike))]
    if files:       # the files of the call are one decode batch
        for k, img in zip(files, imread([imgs[k] for k in files], device=device)):
            imgs[k] = img
    batch, metas = pipe(imgs)
    with torch.no_grad():
        if isinstance(batch, list):      # test-time augmentation: one batch per augmentation (N images each)
            results = model.aug_test(batch, metas, rescale=True)
        else:
            results = model.simple_test(batch, metas, rescale=True)
    return results if is_batch else results[0]


def _unwrap(field):
    """A test-time batch carries one entry per augmentation (``img=[tensor]``, ``img_metas=[[meta, ...]]``); with one
    augmentation the path is ``BaseDetector.forward_test`` -> ``simple_test`` (mmdet/models/detectors/base.py:128-166)."""
    if isinstance(field, (list, tuple)) and len(field) == 1 and isinstance(field[0], (list, tuple, torch.Tensor)):
        return field[0]
    return field


def _test_batches(data_loader, device):
    """``(img, img_metas, tta)`` per batch of a test loader: ``tta`` batches keep one entry per augmentation
    (BaseDetector.forward_test -> aug_test, detectors/base.py:147-153).  The flat loop's copy of the unwrapping that
    ``single_gpu_test``'s list loop keeps inline: that loop is the yardstick the flat one is measured against and stays
    as it was, so a change to the batch format has to be made in both."""
    for data in data_loader:
        img, metas = data['img'], data['img_metas']
        if isinstance(img, (list, tuple)) and len(img) > 1:
            yield [t.to(device, non_blocking=True) for t in img], list(metas), True
        else:
            yield _unwrap(img).to(device, non_blocking=True), _unwrap(metas), False


def _flat_loop(model, data_loader, position):
    """The test loop with the result table built on the device (``results.DeviceResults``): ``position(j)`` is the
    dataset position of the loop's j-th image.  Per batch the host reads the (N,) counts and nothing else;
    test-time-augmentation batches come back as lists (``aug_test``) and are uploaded once."""
    from .results import DeviceResults
    model.eval()
    device = next(model.parameters()).device
    table = DeviceResults(model.bbox_head.num_classes, device)
    seen = 0
    with torch.no_grad():
        for img, metas, tta in _test_batches(data_loader, device):
            n = len(metas[0]) if tta else len(metas)
            index = [position(seen + j) for j in range(n)]
            if tta:
                table.append_lists(model.forward_test(img, metas, rescale=True), index)
            else:
                model.simple_test(img, metas, rescale=True, results=table, img_index=index)
            seen += n
    return table.tensors()


def _show_metas(metas):
    """The per-image metas of a batch: a test-time-augmentation batch nests them per augmentation."""
    return metas[0] if metas and isinstance(metas[0], (list, tuple)) else metas


def _show_batch(model, metas, batch_results, out_dir, score_thr):
    """The visualisation branch of the reference's loop (``mmdet/apis/test.py:30-57``) for one batch: the ORIGINAL files
    (``img_meta['filename']``) are decoded, drawn on and written to ``out_dir / ori_filename`` in one ``show_results``
    call.  The reference draws on the de-normalised network input resized back to the original size; the boxes are in
    original coordinates either way."""
    metas = _show_metas(metas)
    for m in metas:
        for key in ('filename', 'ori_filename'):
            if not m.get(key):
                raise ValueError(f"single_gpu_test(out_dir=...) reads the picture from img_meta[{key!r}], which this "
                                 'batch does not carry')
    model.show_results([m['filename'] for m in metas], batch_results,
                       [os.path.join(out_dir, m['ori_filename']) for m in metas], score_thr=score_thr)


def single_gpu_test(model, data_loader, flat=False, show=False, out_dir=None, show_score_thr=0.3):
    """Run the detector over ``data_loader`` and return the list of per-image results
    (``mmdet/apis/test.py:16-68``).  Each item is ``dict(img=..., img_metas=...)``
    as the test pipeline's collate produces; ``rescale=True`` like the reference's test loop.

    ``out_dir``: every image is drawn with its detections above ``show_score_thr`` and written to ``out_dir /
    img_meta['ori_filename']`` (a JPEG), one decode, draw and encode call per batch (``show_results``); the picture
    drawn on is the original file, not the de-normalised network input.  ``show=True`` raises: there is no display.

    ``flat=True`` returns the flat form instead -- ``(dets (D, 5) float32, labels (D,) int64, img_index (D,) int64)`` as
    GPU tensors, ``img_index`` the running image number -- equal to ``coco_eval.flatten_results`` of the list bit for
    bit, without the detections leaving the device."""
    if show:
        raise NotImplementedError('single_gpu_test(show=True): there is no display window; pass out_dir=')
    if flat and out_dir is not None:
        raise ValueError('single_gpu_test(flat=True, out_dir=...): drawing from the flat result table is not built')
    if flat:
        return _flat_loop(model, data_loader, lambda j: j)
    model.eval()
    device = next(model.parameters()).device
    results = []
    with torch.no_grad():
        for data in data_loader:
            img, metas = data['img'], data['img_metas']
            if isinstance(img, (list, tuple)) and len(img) > 1:
                # test-time augmentation: BaseDetector.forward_test -> aug_test (detectors/base.py:147-153)
                results.extend(model.forward_test([t.to(device, non_blocking=True) for t in img], list(metas),
                                                  rescale=True))
            else:
                img, metas = _unwrap(img), _unwrap(metas)
                results.extend(model.simple_test(img.to(device, non_blocking=True), metas, rescale=True))
            if out_dir is not None:
                _show_batch(model, list(metas), results[len(results) - len(_show_metas(metas)):], out_dir, show_score_thr)
    return results


def multi_gpu_test(model, data_loader, size=None, gpu_collect=True, flat=False):
    """Every rank runs its ``sampler_indices`` share, then rank 0 receives the merged, dataset-ordered list and the
    others ``None`` (``mmdet/apis/test.py:71-113``).  ``size`` defaults to ``len(data_loader.dataset)``.  With
    ``gpu_collect`` the byte buffers of the gather live on the rank's GPU (RCCL); otherwise on the host (gloo) --
    the reference's other branch goes through a shared temp directory instead.

    ``flat=True``: the flat form of ``single_gpu_test``.  Rank r's j-th image sits at dataset position ``j * world + r``
    (the sampler's round-robin deal), ``dist.collect_flat`` gathers the three tensors and rank 0 returns them ordered
    by position, without the sampler's padding, on the model's device."""
    from . import dist as D
    if size is None:
        size = len(data_loader.dataset)
    device = next(model.parameters()).device if gpu_collect else 'cpu'
    if flat:
        rank, world = D.rank_world()
        dets, labels, img_index = _flat_loop(model, data_loader, lambda j: j * world + rank)
        return D.collect_flat(dets, labels, img_index, size, device=device)
    results = single_gpu_test(model, data_loader)
    return D.collect_results(results, size, device=device)
