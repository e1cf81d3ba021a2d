"""ctypes binding of ``libyv4_hip.so`` (the C-ABI declared in ``include/yv4.h``).

The library is the product: there is no CPU fallback.  ``lib()`` raises
``RuntimeError`` when the shared object has not been built, and every wrapper
raises on a non-zero status with the library's own error message.
"""
import collections
import ctypes as C
import os
import subprocess
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_DIR = os.path.join(_HERE, 'lib')
LIB_PATH = os.environ.get('YV4_LIB_PATH') or os.path.join(LIB_DIR, 'libyv4_hip.so')   # override: A/B measurement builds
CSRC_DIR = os.path.join(_HERE, 'csrc')

# ---- constants mirrored from include/yv4.h -------------------------------------
ABI_VERSION = 8
STATS_REPLICAS = 64        # YV4_STATS_REPLICAS
GRAD_PREPARE_MAX_WG = 2048  # YV4_GRAD_PREPARE_MAX_WG
F32, F16, BF16, F64 = 0, 1, 2, 3
DTYPE_CODE = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16}    # the element code of a tensor's dtype
F8E4M3 = 3                 # YV4_F8E4M3: the fp8 entry points' element code (the standalone op's F64 elsewhere)
F8TILE_128x128, F8TILE_128x64, F8TILE_64x64 = 1, 2, 3
ACT_NONE, ACT_MISH, ACT_LEAKY, ACT_SWISH = 0, 1, 2, 3
NMS_IOU_DIV, NMS_IOU_MUL = 0, 1
OVERLAPS_IOU, OVERLAPS_IOF = 0, 1                                           # YV4_OVERLAPS_*
TPFP_DEFAULT, TPFP_IMAGENET = 0, 1                                          # YV4_TPFP_*
MAP_AP_AREA, MAP_AP_11POINTS = 0, 1                                         # YV4_MAP_AP_*
SOFT_NMS_NAIVE, SOFT_NMS_LINEAR, SOFT_NMS_GAUSSIAN = 0, 1, 2                # YV4_SOFT_NMS_*
SOFT_NMS_METHODS = {'naive': SOFT_NMS_NAIVE, 'linear': SOFT_NMS_LINEAR, 'gaussian': SOFT_NMS_GAUSSIAN}
FLIP_NONE, FLIP_HORIZONTAL, FLIP_VERTICAL, FLIP_DIAGONAL = 0, 1, 2, 3     # YV4_FLIP_*
FLIP_CODES = {'horizontal': FLIP_HORIZONTAL, 'vertical': FLIP_VERTICAL, 'diagonal': FLIP_DIAGONAL}
TTA_MAX_AUGS = 16          # YV4_TTA_MAX_AUGS
V3AUG_CONTRAST_NONE, V3AUG_CONTRAST_FIRST, V3AUG_CONTRAST_LAST = 0, 1, 2    # YV4_V3AUG_CONTRAST_*
TILE_AUTO, TILE_128x128, TILE_128x64, TILE_64x64, TILE_64x128 = 0, 1, 2, 3, 4
TILE_DMA_64x64, TILE_DMA_128x64, TILE_DMA_128x128, TILE_STEM, TILE_WS_1x1 = 5, 6, 7, 8, 9
TILE_W3x3, TILE_WIDE = 10, 11
CONV_NT_OUT = 1            # yv4_conv_desc.flags (ABI 7): non-temporal output stores
HTILE_NAMES = {1: 'h16_128x128', 2: 'h16_128x64', 3: 'h16_64x64', 4: 'h16_pp3x3', 5: 'h16_w3x3', 6: 'h16_ws_1x1', 7: 'h16_s3x3', 8: 'h16_wide'}
TILE_NAMES = {0: 'auto', 1: '128x128', 2: '128x64', 3: '64x64', 4: '64x128', 5: 'dma64x64', 6: 'dma128x64',
              7: 'dma128x128', 8: 'stem3x3', 9: 'ws_1x1', 10: 'w3x3', 11: 'wide'}
#: how many workgroup-tile shapes each ``YV4_*_SHAPE(i)`` macro pins (tests, tile sweeps): i = 0 .. count - 1
SHAPE_COUNTS = {'TILE_W3x3': 5, 'TILE_WIDE': 5, 'HTILE_W3x3': 7, 'HTILE_WIDE': 5}
# YV4_TILE_x_SHAPE(i) = x + 16 * (i + 1), YV4_HTILE_x_SHAPE(i) = x + 8 * (i + 1): same kernels, same names
TILE_NAMES.update({TILE_W3x3 + 16 * (i + 1): 'w3x3' for i in range(SHAPE_COUNTS['TILE_W3x3'])})
TILE_NAMES.update({TILE_WIDE + 16 * (i + 1): 'wide' for i in range(SHAPE_COUNTS['TILE_WIDE'])})
HTILE_NAMES.update({5 + 8 * (i + 1): 'h16_w3x3' for i in range(SHAPE_COUNTS['HTILE_W3x3'])})
HTILE_NAMES.update({8 + 8 * (i + 1): 'h16_wide' for i in range(SHAPE_COUNTS['HTILE_WIDE'])})
E_INVALID, E_UNSUPPORTED = -1, -2                                           # YV4_E_*: the status of a refused call
LOSS_MAX_LEVELS = V3_LOSS_MAX_LEVELS = 5


class ConvDesc(C.Structure):
    """``yv4_conv_desc``."""
    _fields_ = [(n, C.c_int32) for n in (
        'N', 'H', 'W', 'Cin', 'Ho', 'Wo', 'Cout', 'KH', 'KW', 'stride', 'pad',
        'x_cstride', 'x_coff', 'y_cstride', 'y_coff', 'r_cstride', 'r_coff',
        'act1', 'act2')] + [('slope1', C.c_float), ('slope2', C.c_float),
                            ('tile', C.c_int32), ('flags', C.c_int32)]


class LevelDesc(C.Structure):
    """``yv4_level_desc``."""
    _fields_ = [('pred', C.c_void_p), ('H', C.c_int32), ('W', C.c_int32),
                ('stride', C.c_int32), ('base_anchors', (C.c_float * 4) * 8)]


class TtaAug(C.Structure):
    """``yv4_tta_aug``."""
    _fields_ = [('boxes', C.c_void_p), ('conf', C.c_void_p), ('cls', C.c_void_p), ('slots', C.c_void_p),
                ('total', C.c_int64), ('S', C.c_int32), ('flip', C.c_int32)]


class LossLevel(C.Structure):
    """``yv4_loss_level``."""
    _fields_ = [('raw', C.c_void_p), ('draw', C.c_void_p), ('bias', C.c_void_p), ('dbias', C.c_void_p),
                ('H', C.c_int32), ('W', C.c_int32), ('Cp', C.c_int32), ('stride', C.c_int32),
                ('base_anchors', (C.c_float * 4) * 8)]


class LossDesc(C.Structure):
    """``yv4_loss_desc``."""
    _fields_ = [('levels', LossLevel * LOSS_MAX_LEVELS),
                ('num_levels', C.c_int32), ('N', C.c_int32), ('A', C.c_int32), ('num_classes', C.c_int32),
                ('G', C.c_int32), ('dtype', C.c_int32),
                ('gt', C.c_void_p), ('gt_label', C.c_void_p), ('gt_img', C.c_void_p),
                ('shape_thr', C.c_float), ('smooth', C.c_float), ('ratio', C.c_float), ('eps', C.c_float),
                ('w_cls', C.c_float), ('w_conf', C.c_float), ('w_bbox', C.c_float),
                ('slot_anchor', C.c_void_p), ('winner', C.c_void_p), ('npos', C.c_void_p), ('conf_t', C.c_void_p),
                ('gpos', C.c_void_p), ('sums', C.c_void_p), ('losses', C.c_void_p)]


class LossOpts(C.Structure):
    """``yv4_loss_opts``: the box loss and the SoftFocalLoss switches of ``yv4_yolo_loss_fwd_ex`` / ``_bwd_ex``."""
    _fields_ = [('box_kind', C.c_int32), ('conf_focal', C.c_int32), ('conf_gamma', C.c_float), ('conf_alpha', C.c_float),
                ('cls_focal', C.c_int32), ('cls_gamma', C.c_float), ('cls_alpha', C.c_float), ('reserved', C.c_int32 * 9)]


#: ``yv4_loss_opts.box_kind`` (YV4_BOX_* in include/yv4.h)
BOX_GIOU, BOX_IOU_LINEAR, BOX_IOU_LOG, BOX_DIOU, BOX_CIOU = range(5)


class V3LossLevel(C.Structure):
    """``yv4_v3_loss_level`` (ABI 8)."""
    _fields_ = [('pred', C.c_void_p), ('dpred', C.c_void_p),
                ('sn', C.c_int64), ('sc', C.c_int64), ('sh', C.c_int64), ('sw', C.c_int64),
                ('H', C.c_int32), ('W', C.c_int32), ('stride', C.c_int32), ('reserved', C.c_int32),
                ('base_anchors', (C.c_float * 4) * 8)]


class V3LossDesc(C.Structure):
    """``yv4_v3_loss_desc`` (ABI 8)."""
    _fields_ = [('levels', V3LossLevel * V3_LOSS_MAX_LEVELS),
                ('num_levels', C.c_int32), ('N', C.c_int32), ('A', C.c_int32), ('num_classes', C.c_int32),
                ('G', C.c_int32), ('gt_max_assign_all', C.c_int32),
                ('gt', C.c_void_p), ('gt_label', C.c_void_p), ('gt_img', C.c_void_p),
                ('pos_iou_thr', C.c_float), ('neg_lo', C.c_float), ('neg_hi', C.c_float), ('min_pos_iou', C.c_float),
                ('eps', C.c_float), ('eps_hi', C.c_float), ('iou_eps', C.c_float), ('smoother', C.c_float),
                ('loss_weight', C.c_float * 4), ('reduce_mean', C.c_int32 * 4),
                ('img_off', C.c_void_p), ('gt_cell', C.c_void_p), ('gt_max', C.c_void_p), ('gt_arg', C.c_void_p),
                ('assigned', C.c_void_p), ('sums', C.c_void_p), ('losses', C.c_void_p)]


class AugImage(C.Structure):
    """``yv4_aug_image``."""
    _fields_ = [('src', C.c_void_p * 4), ('sh', C.c_int32 * 4), ('sw', C.c_int32 * 4), ('pitch', C.c_int32 * 4),
                ('rh', C.c_int32 * 4), ('rw', C.c_int32 * 4)] + \
               [(n, C.c_int32) for n in ('cxy', 'left', 'top', 'x1', 'y1', 'C', 'S', 'o', 'flip', 'hsv_on')] + \
               [('lut', (C.c_uint8 * 256) * 3)]


class V3AugImage(C.Structure):
    """``yv4_v3aug_image``."""
    _fields_ = [('src', C.c_void_p)] + \
               [(n, C.c_int32) for n in ('sh', 'sw', 'pitch', 'bright_on', 'contrast_mode', 'sat_on', 'hue_on', 'perm_on')] + \
               [(n, C.c_float) for n in ('bright_delta', 'contrast_alpha', 'sat_alpha', 'hue_delta')] + \
               [('perm', C.c_int32 * 3)] + [(n, C.c_int32) for n in ('eh', 'ew', 'etop', 'eleft')] + \
               [('fill', C.c_float * 3)] + \
               [(n, C.c_int32) for n in ('cx', 'cy', 'cw', 'ch', 'rh', 'rw', 'ph', 'pw', 'flip', 'reserved')]


class LetterboxSlot(C.Structure):
    """``yv4_letterbox_slot``: one (augmentation, image) slot of a ``yv4_letterbox_u8_batch`` call."""
    _fields_ = [('src', C.c_void_p), ('inv_sx', C.c_double), ('inv_sy', C.c_double), ('dst_off', C.c_int64)] + \
               [(n, C.c_int32) for n in ('src_h', 'src_w', 'src_pitch', 'new_h', 'new_w', 'pad_h', 'pad_w', 'H', 'W', 'flip')]


class PackDesc(C.Structure):
    """yv4_pack_desc (include/yv4.h)."""
    _fields_ = [('w', C.c_void_p), ('s_co', C.c_int64), ('s_ci', C.c_int64), ('s_kh', C.c_int64), ('s_kw', C.c_int64),
                ('dst', C.c_void_p)] + [(k, C.c_int32) for k in (
                    'Cout', 'Cin', 'KHo', 'KWo', 'kh0', 'kh_step', 'kw0', 'kw_step', 'transpose', 'pad_to', 'dtype',
                    'first_block', 'nblocks', 'rows_per_block')]


class JpegInfo(C.Structure):
    """``yv4_jpeg_info``: what the host half of the JPEG decoder reads from a file's headers."""
    _fields_ = [(n, C.c_int32) for n in ('width', 'height', 'ncomp')] + \
               [(n, C.c_int32 * 3) for n in ('hs', 'vs', 'tq', 'td', 'ta')] + \
               [(n, C.c_int32) for n in ('restart_interval', 'mcus_x', 'mcus_y')] + \
               [('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3), ('orientation', C.c_int32),
                ('ncoef', C.c_int64), ('scan_offset', C.c_int64), ('quant', (C.c_uint16 * 64) * 4)]


class JpegImage(C.Structure):
    """``yv4_jpeg_image``: one image of a ``yv4_jpeg_reconstruct`` call."""
    _fields_ = [('coef_off', C.c_int64), ('plane_off', C.c_int64 * 3), ('out_off', C.c_int64),
                ('unit_base', C.c_int64), ('tile_base', C.c_int64)] + \
               [(n, C.c_int32) for n in ('out_pitch', 'width', 'height', 'ncomp', 'hs', 'vs')] + \
               [('tq', C.c_int32 * 3), ('blocks_w', C.c_int32 * 3), ('blocks_h', C.c_int32 * 3), ('orientation', C.c_int32)]


class JpegHuff(C.Structure):
    """``yv4_jpeg_huff``: one Huffman table in the form the scan decode reads."""
    _fields_ = [('look', C.c_uint16 * 512), ('maxcode', C.c_int32 * 8), ('valoff', C.c_int32 * 8), ('vals', C.c_uint8 * 256)]


class JpegScan(C.Structure):
    """``yv4_jpeg_scan``: one image of a ``yv4_jpeg_entropy_decode_device`` call."""
    _fields_ = [(n, C.c_int64) for n in ('data_off', 'data_len', 'coef_off', 'ncoef', 'seg_base')] + \
               [(n, C.c_int32) for n in ('nseg', 'ncomp', 'mcus_x', 'mcus_y', 'hs', 'vs')] + \
               [('td', C.c_int32 * 3), ('ta', C.c_int32 * 3), ('huff_base', C.c_int32), ('nhuff', C.c_int32)]


class JpegSegment(C.Structure):
    """``yv4_jpeg_segment``: a run of whole MCUs that decodes on its own."""
    _fields_ = [('begin', C.c_int64), ('end', C.c_int64)] + \
               [(n, C.c_int32) for n in ('first_mcu', 'mcu_count', 'bit_off', 'reserved')] + [('pred', C.c_int16 * 4)]


class JpegWg(C.Structure):
    """``yv4_jpeg_wg``: the segments one workgroup of the scan decode serves."""
    _fields_ = [(n, C.c_int32) for n in ('image', 'first_seg', 'count', 'reserved')]


class JpegChunk(C.Structure):
    """``yv4_jpeg_chunk``: one chunk of a segment's bytes, the unit of the self-synchronising scan decode."""
    _fields_ = [(n, C.c_int32) for n in ('image', 'seg', 'index', 'count')]


class JpegEntry(C.Structure):
    """``yv4_jpeg_entry``: the state a chunk was decoded from and what the pass left."""
    _fields_ = [('entry', C.c_uint64), ('exit', C.c_uint64 * 2), ('nblk', C.c_int32), ('first_block', C.c_int32),
                ('dc', C.c_uint16 * 3), ('tail', C.c_uint16), ('pred', C.c_int16 * 3), ('reserved', C.c_int16)]


#: ``YV4_JPEG_MAX_HUFF`` / ``YV4_JPEG_WG_SEGMENTS`` (include/yv4.h)
JPEG_MAX_HUFF, JPEG_WG_SEGMENTS = 6, 64


class JpegEncImage(C.Structure):
    """``yv4_jpeg_enc_image``: one image of a JPEG encode call."""
    _fields_ = [(n, C.c_int64) for n in ('src_off', 'coef_off', 'work_off', 'out_off', 'out_cap', 'wg_base', 'swg_base',
                                         'nblocks')] + \
               [(n, C.c_int32) for n in ('src_pitch', 'width', 'height', 'channels', 'ncomp', 'hs', 'vs', 'quality',
                                         'mcus_x', 'mcus_y')] + \
               [(n, C.c_int32 * 3) for n in ('blocks_w', 'blocks_h', 'real_w', 'real_h')] + [('quant', (C.c_uint16 * 64) * 2)]


class DrawImage(C.Structure):
    """``yv4_draw_image``: one image of a ``yv4_draw_boxes`` call."""
    _fields_ = [(n, C.c_int64) for n in ('pix_off', 'box_base', 'wg_base')] + \
               [(n, C.c_int32) for n in ('pitch', 'width', 'height', 'nbox')]


class DrawStyle(C.Structure):
    """``yv4_draw_style``."""
    _fields_ = [('bbox_color', C.c_int32 * 3), ('text_color', C.c_int32 * 3), ('thickness', C.c_int32),
                ('font_size', C.c_int32), ('num_classes', C.c_int32), ('score_thr', C.c_float)]


#: ``YV4_DRAW_NAME_BYTES`` (include/yv4.h): a row of the class-name table, its first byte the length
DRAW_NAME_BYTES = 32
#: ``YV4_JPEG_ENC_WG_BLOCKS`` / ``YV4_JPEG_ENC_BLOCK_BITS`` / ``YV4_JPEG_ENC_HEADER_MAX`` (include/yv4.h): the blocks one
#: workgroup of the encoder's bit-offset scan covers, the bound on a block's bits, the room the header writer asks for
JPEG_ENC_WG_BLOCKS, JPEG_ENC_BLOCK_BITS, JPEG_ENC_HEADER_MAX = 256, 1660, 640

#: every struct of include/yv4.h: C type name -> its ctypes mirror (tests/_abi_probe.py checks each field with a C compiler)
STRUCTS = {
    'yv4_conv_desc': ConvDesc, 'yv4_level_desc': LevelDesc, 'yv4_tta_aug': TtaAug, 'yv4_loss_level': LossLevel,
    'yv4_loss_desc': LossDesc, 'yv4_loss_opts': LossOpts, 'yv4_v3_loss_level': V3LossLevel, 'yv4_v3_loss_desc': V3LossDesc,
    'yv4_aug_image': AugImage, 'yv4_v3aug_image': V3AugImage, 'yv4_letterbox_slot': LetterboxSlot, 'yv4_pack_desc': PackDesc,
    'yv4_jpeg_info': JpegInfo, 'yv4_jpeg_image': JpegImage, 'yv4_jpeg_huff': JpegHuff, 'yv4_jpeg_scan': JpegScan,
    'yv4_jpeg_segment': JpegSegment, 'yv4_jpeg_wg': JpegWg, 'yv4_jpeg_chunk': JpegChunk, 'yv4_jpeg_entry': JpegEntry,
    'yv4_jpeg_enc_image': JpegEncImage, 'yv4_draw_image': DrawImage, 'yv4_draw_style': DrawStyle,
}

_vp, _i, _i64, _f, _sz, _d = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t, C.c_double

#: every exported symbol: name -> (restype, argtypes).  tests/test_abi.py checks
#: this table against include/yv4.h and against the built library.
SIGNATURES = {
    'yv4_abi_version': (C.c_int, []),
    'yv4_last_error': (C.c_char_p, []),
    'yv4_arch': (C.c_char_p, []),
    'yv4_mish_fwd': (C.c_int, [_vp, _vp, _sz, _i, _vp]),
    'yv4_mish_bwd': (C.c_int, [_vp, _vp, _vp, _sz, _i, _vp]),
    'yv4_mish_fwd_host': (C.c_int, [_vp, _vp, _sz, _i]),
    'yv4_mish_bwd_host': (C.c_int, [_vp, _vp, _vp, _sz, _i]),
    'yv4_nchw_to_nhwc': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_nhwc_to_nchw': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_conv_bn_act_fwd': (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _vp]),
    'yv4_conv_splitk_workspace': (_sz, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    'yv4_conv_bn_act_fwd_splitk': (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'yv4_conv_h16_splitk_workspace': (_sz, [C.POINTER(ConvDesc), C.POINTER(C.c_int)]),
    'yv4_conv_bn_act_fwd_h16_splitk': (C.c_int, [C.POINTER(ConvDesc), C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    'yv4_conv_flops': (C.c_double, [C.POINTER(ConvDesc)]),
    'yv4_conv_pick_tile': (C.c_int, [C.POINTER(ConvDesc)]),
    'yv4_spp_pool_fwd': (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_resample_nearest_fwd': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i,
                                           _i, _i, _i, _i, _vp]),
    'yv4_resample_nearest_bwd': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_decode_reset': (C.c_int, [_vp, _vp, _i, _vp]),
    'yv4_decode_filter': (C.c_int, [C.POINTER(LevelDesc), _i, _i, _i, _i, _f,
                                    _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp,
                                    _vp, _vp]),
    'yv4_decode_filter_v3': (C.c_int, [C.POINTER(LevelDesc), _i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _i64, _vp,
                                       _vp, _vp, _vp]),
    'yv4_conf_topk_levels_work': (_sz, [_i, _i64, _i]),
    'yv4_conf_topk_levels': (C.c_int, [C.POINTER(LevelDesc), _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'yv4_conf_topk_work': (_sz, [_i, _i64]),
    'yv4_conf_topk': (C.c_int, [C.POINTER(LevelDesc), _i, _i, _i, _i, _i, _vp, _vp, _vp]),
    'yv4_nms_images': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i,
                                 _i, _f, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    'yv4_nms_split_work': (_sz, [_i64]),
    'yv4_nms_split': (C.c_int, [_vp, _i64, _f, _vp, _vp, _i, _f, _i, _vp, _vp,
                                _vp, _vp, _vp, _vp]),
    'yv4_nms_prepare': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    'yv4_nms_set_iou_form': (C.c_int, [_i]),
    'yv4_set_deterministic': (C.c_int, [_i]),
    'yv4_get_deterministic': (C.c_int, []),
    'yv4_conv_stats_fold': (C.c_int, [_vp, _i, _i, _vp, _vp]),
    'yv4_nms_get_iou_form': (C.c_int, []),
    'yv4_conv_wgrad': (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp]),
    'yv4_conv_wgrad_workspace': (_sz, [C.POINTER(ConvDesc), _i]),
    'yv4_conv_wgrad_det': (C.c_int, [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    'yv4_dilate2_fwd': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_bn_train_stats': (C.c_int, [_vp, _i64, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_bn_act_fwd': (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _i, _i, _f, _vp]),
    'yv4_bn_act_bwd': (C.c_int, [_vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64, _i,
                                 _i, _f, _vp]),
    'yv4_conv_bn_act_fwd_h16': (C.c_int, [C.POINTER(ConvDesc), _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_conv_stem_fwd': (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'yv4_conv_h16_pick_tile': (C.c_int, [C.POINTER(ConvDesc)]),
    'yv4_stem_down_fwd_h16': (C.c_int, [_i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _vp, _i, _i, _f, _vp, _i, _i,
                                        _vp]),
    'yv4_nchw_to_nhwc_h16': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_nhwc_to_nchw_h16': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_spp_pool_fwd_h16': (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_conv_wgrad_h16': (C.c_int, [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp]),
    'yv4_bn_train_stats_h16': (C.c_int, [_vp, _i, _i64, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_bn_act_fwd_h16': (C.c_int, [_vp, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i, _i, _i64, _i, _i, _f,
                                     _vp]),
    'yv4_bn_act_bwd_h16': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64,
                                     _i, _i, _f, _vp]),
    'yv4_conv_scatter_fwd': (C.c_int, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_conv_scatter_fwd_h16': (C.c_int, [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_bn_eval_act_bwd': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64,
                                      _i, _i, _f, _vp]),
    'yv4_spp_pool_bwd': (C.c_int, [_vp, _i, _i, _vp, _i, _i, _vp, _i, _i, _i, _i, _i, _vp]),
    'yv4_bn_act_bwd_accum': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp, _i64, _i, _i, _f, _i, _vp]),
    'yv4_bn_partial_sums': (C.c_int, [_vp, _i, _i64, _i, _i, _i, _vp, _vp]),
    'yv4_bn_finalize': (C.c_int, [_vp, _i, _i64, _vp, _i, _f, _f, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    'yv4_conv_fwd_stats': (C.c_int, [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    'yv4_bn_act_bwd_sums': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _f, _vp]),
    'yv4_bn_act_bwd_apply': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _i64, _i64, _vp, _i, _i, _f, _vp]),
    'yv4_pack_weight': (C.c_int, [_vp, _i64, _i64, _i64, _i64] + [_i] * 12 + [_vp, _i, _vp]),
    'yv4_pack_weights_multi': (C.c_int, [_vp, _i, _i, _vp]),
    'yv4_yolo_loss_fwd': (C.c_int, [C.POINTER(LossDesc), _vp]),
    'yv4_yolo_loss_bwd': (C.c_int, [C.POINTER(LossDesc), _vp, _vp]),
    'yv4_yolo_loss_fwd_ex': (C.c_int, [C.POINTER(LossDesc), C.POINTER(LossOpts), _vp]),
    'yv4_yolo_loss_bwd_ex': (C.c_int, [C.POINTER(LossDesc), C.POINTER(LossOpts), _vp, _vp]),
    'yv4_yolov3_loss_fwd': (C.c_int, [C.POINTER(V3LossDesc), _vp]),
    'yv4_yolov3_loss_bwd': (C.c_int, [C.POINTER(V3LossDesc), _vp, _vp]),
    'yv4_mosaic_augment_u8': (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    'yv4_augment_boxes': (C.c_int, [_vp, _i, _i, _vp, _vp, _vp, _vp, _i, _d, _d, _f, _f, _vp, _vp, _vp, _vp]),
    'yv4_letterbox_u8': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _i, _i, _i, _vp]),
    'yv4_iou_coco_batched': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _vp, _vp]),
    'yv4_match_coco_batched': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    'yv4_grad_prepare': (C.c_int, [_vp, _i64, _vp, _f, _vp, _vp, _vp]),
    'yv4_sgd_step': (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _i, _vp, _vp]),
    'yv4_loss_scale_update': (C.c_int, [_vp, _vp, _f, _f, _i, _vp]),
    'yv4_ema_update': (C.c_int, [_vp, _vp, _i64, _f, _vp]),
    'yv4_conv_bn_act_fwd_f8': (C.c_int, [C.POINTER(ConvDesc), _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _vp, _vp]),
    'yv4_conv_f8_pick_tile': (C.c_int, [C.POINTER(ConvDesc)]),
    'yv4_quantize_f8': (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _i, _f, _vp]),
    'yv4_spp_pool_fwd_f8': (C.c_int, [_vp, _i, _i, _i, _i, _i, _i, _vp]),
    'yv4_letterbox_u8_flip': (C.c_int, [_vp, _i, _i, _i, _vp, _i, _i, _i64, _i, _i, _vp, _vp, _i, _i, _i, _i, _vp]),
    'yv4_letterbox_u8_batch': (C.c_int, [C.POINTER(LetterboxSlot), _vp, _i, _vp, _i64, _vp, _vp, _i, _i, _i, _vp]),
    'yv4_topk_slots_work': (_sz, [_i, _vp, _i]),
    'yv4_topk_slots': (C.c_int, [_vp, _i, _i64, _i, _vp, _i, _vp, _vp, _vp, _i64, _vp]),
    'yv4_tta_merge': (C.c_int, [C.POINTER(TtaAug), _i, _i, _i, _f, _vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    'yv4_soft_nms_images': (C.c_int, [_vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i, _i, _i, _f, _f, _f, _i, _i, _vp, _vp,
                                      _vp, _vp, _vp]),
    'yv4_soft_nms_split_work': (_sz, [_i64]),
    'yv4_soft_nms_split': (C.c_int, [_vp, _i64, _f, _vp, _vp, _i, _i, _i, _f, _f, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_v3_augment_u8': (C.c_int, [_vp, _i, _vp, _i, _i, _vp, _vp, _i, _vp]),
    'yv4_bbox_overlaps_batched': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i, _f, _vp, _vp]),
    'yv4_tpfp_work': (_sz, [_i, _i64, _i64, _i]),
    'yv4_tpfp_batched': (C.c_int, [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _vp, _vp, _i, _vp, _i,
                                   _vp, _vp, _vp, _vp]),
    'yv4_map_rank_work': (_sz, [_i64]),
    'yv4_map_rank': (C.c_int, [_vp, _vp, _vp, _i64, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_map_accumulate_work': (_sz, [_i64, _i, _i]),
    'yv4_map_accumulate': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                     _vp]),
    'yv4_map_image_ap_work': (_sz, [_i64]),
    'yv4_map_image_ap': (C.c_int, [_vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _i, _i, _i, _vp, _sz, _vp, _i64, _vp, _i64,
                                   _vp]),
    'yv4_map_image_mean': (C.c_int, [_vp, _i64, _vp, _i64, _i, _i, _i, _vp, _i64, _vp, _i64, _vp]),
    'yv4_recall_work': (_sz, [_i64, _i64, _i, _i]),
    'yv4_recall_match': (C.c_int, [_vp, _vp, _vp, _vp, _i64, _i, _i64, _i64, _vp, _i, _vp, _i, C.c_float, _i, _vp, _sz, _vp,
                                   _i64, _vp, _i64, _vp]),
    'yv4_flex_tables': (C.c_int, [_vp, _vp, _i, _i, _vp, _vp, _vp]),
    'yv4_flex_accumulate_work': (_sz, [_i64, _i, _i]),
    'yv4_flex_accumulate': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _i, _i, _i, _i, _i, _vp, _vp, _vp,
                                      _vp, _vp]),
    'yv4_coco_rank_work': (_sz, [_i64]),
    'yv4_coco_rank': (C.c_int, [_vp, _vp, _i64, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    'yv4_coco_match': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _i, _vp, _i, _vp, _i, _vp, _i64, _vp, _vp,
                                 _vp, _vp]),
    'yv4_coco_accumulate_work': (_sz, [_i64, _i, _i]),
    'yv4_coco_accumulate': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _vp, _i, _i, _i, _vp, _i, _vp, _vp, _vp,
                                      _vp, _vp]),
    'yv4_coco_error_need': (C.c_int, [_vp, _vp, _i, _i, _i, _i, _vp, _vp]),
    'yv4_coco_error_match': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i64, _i64, _i, _vp, _i, _d, _vp,
                                       _i, _vp, _i64, _vp, _vp, _vp, _vp]),
    'yv4_results_append': (C.c_int, [_vp, _vp, _vp, _vp, _i, _i, _i, _i64, _i64, _vp, _vp, _vp, _vp]),
    'yv4_jpeg_parse': (C.c_int, [_vp, _sz, C.POINTER(JpegInfo)]),
    'yv4_jpeg_entropy_decode': (C.c_int, [_vp, _sz, C.POINTER(JpegInfo), _vp, _i64]),
    'yv4_jpeg_layout': (C.c_int, [C.POINTER(JpegInfo), _i, C.POINTER(JpegImage), C.POINTER(C.c_int64)]),
    'yv4_jpeg_layout_oriented': (C.c_int, [C.POINTER(JpegInfo), _i, _i, C.POINTER(JpegImage), C.POINTER(C.c_int64)]),
    'yv4_jpeg_reconstruct': (C.c_int, [C.POINTER(JpegImage), _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i, _vp]),
    'yv4_jpeg_scan_prepare': (C.c_int, [_vp, _sz, C.POINTER(JpegInfo), _vp, _vp, _vp, _i64]),
    'yv4_jpeg_entropy_workgroups': (C.c_int, [_vp, _i, _vp, _i64, C.POINTER(C.c_int64)]),
    'yv4_jpeg_entropy_decode_segments': (C.c_int, [_vp, _vp, _vp, _i, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    'yv4_jpeg_entropy_decode_device': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _vp, _i64, _vp, _i64, _vp,
                                                 _i64, _vp, _vp]),
    'yv4_jpeg_entropy_strerror': (C.c_char_p, [_i]),
    'yv4_jpeg_chunks_build': (C.c_int, [_vp, _vp, _i, _i64, C.c_int32, _vp, _i64, _vp, _vp, _i64, C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64)]),
    'yv4_jpeg_entropy_decode_sync': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i64, _vp, _i64, _vp, _i64,
                                               C.c_int32, C.c_int32, _vp, _vp, _i64, _vp, _vp, _vp]),
    'yv4_jpeg_entropy_decode_device_sync': (C.c_int, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i64, _i64, _i64,
                                                      _vp, _i64, _vp, _i64, C.c_int32, C.c_int32, _vp, _vp, _i64, _vp, _vp,
                                                      _vp]),
    'yv4_jpeg_encode_layout': (C.c_int, [C.POINTER(JpegEncImage), _i, C.POINTER(C.c_int64)]),
    'yv4_jpeg_encode_validate': (C.c_int, [C.POINTER(JpegEncImage), _i, _i64, _i64, _i64, _i64]),
    'yv4_jpeg_encode_header': (C.c_int, [C.POINTER(JpegEncImage), _vp, _i64, C.POINTER(C.c_int64)]),
    'yv4_jpeg_encode_host': (C.c_int, [C.POINTER(JpegEncImage), _i, _i, _vp, _i64, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp]),
    'yv4_jpeg_encode_coefficients': (C.c_int, [C.POINTER(JpegEncImage), _vp, _i, _vp, _i64, _i, _vp, _i64, _vp]),
    'yv4_jpeg_encode_scan': (C.c_int, [C.POINTER(JpegEncImage), _vp, _i, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp]),
    'yv4_draw_layout': (C.c_int, [C.POINTER(DrawImage), _i, C.POINTER(C.c_int64)]),
    'yv4_draw_boxes': (C.c_int, [C.POINTER(DrawImage), _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(DrawStyle), _vp]),
    'yv4_draw_boxes_host': (C.c_int, [C.POINTER(DrawImage), _i, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(DrawStyle)]),
    'yv4_draw_boxes_ex': (C.c_int, [C.POINTER(DrawImage), _vp, _i, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(DrawStyle), _i,
                                    _vp]),
    'yv4_draw_boxes_host_ex': (C.c_int, [C.POINTER(DrawImage), _i, _vp, _i64, _vp, _vp, _i64, _vp, C.POINTER(DrawStyle), _i]),
}

Feature = collections.namedtuple('Feature', 'symbols requires abi', defaults=((), 0))

#: the entry points that came after the first ABI-8 build, by feature.  A symbol named here is bound when the library
#: exports it and skipped when it does not, so that an older build still loads for A/B runs (``YV4_LIB_PATH``); every
#: other symbol of ``SIGNATURES`` must exist.  ``has(name)`` says whether all of a feature's symbols, and those of the
#: features it ``requires``, are there.  ``abi``: the feature came with that ABI number instead -- its symbols are bound
#: when the library reports at least that ABI (``YV4_LIB_ABI_ANY=1`` admits the one before), and ``has`` is that test.
FEATURES = {
    # the fp8 (e4m3) inference plans
    'fp8': Feature({'yv4_conv_bn_act_fwd_f8', 'yv4_conv_f8_pick_tile', 'yv4_quantize_f8', 'yv4_spp_pool_fwd_f8'}),
    # the YOLOv3 test-time augmentation
    'tta': Feature({'yv4_letterbox_u8_flip', 'yv4_topk_slots_work', 'yv4_topk_slots', 'yv4_tta_merge'}),
    # a whole test batch's letterbox in one launch
    'letterbox_batch': Feature({'yv4_letterbox_u8_batch'}),
    'soft_nms': Feature({'yv4_soft_nms_images', 'yv4_soft_nms_split_work', 'yv4_soft_nms_split'}),
    # the YOLOv3 train-side input pipeline
    'v3_augment': Feature({'yv4_v3_augment_u8'}),
    # the YOLOCSPHead loss with options: IoU / DIoU / CIoU box terms and SoftFocalLoss
    'loss_ex': Feature({'yv4_yolo_loss_fwd_ex', 'yv4_yolo_loss_bwd_ex'}),
    # the VOC-style mAP, its flat-table ends, and metric='fast-bbox' from the flat table
    'map_eval': Feature({'yv4_bbox_overlaps_batched', 'yv4_tpfp_work', 'yv4_tpfp_batched'}),
    'map_flat': Feature({'yv4_map_rank_work', 'yv4_map_rank', 'yv4_map_accumulate_work', 'yv4_map_accumulate'}),
    'flex_flat': Feature({'yv4_flex_tables', 'yv4_flex_accumulate_work', 'yv4_flex_accumulate'}, ('map_flat',)),
    # the COCO bbox evaluation
    'coco_eval': Feature({'yv4_coco_rank_work', 'yv4_coco_rank', 'yv4_coco_match', 'yv4_coco_accumulate_work',
                          'yv4_coco_accumulate'}),
    # the flat result table of a test loop
    'results_append': Feature({'yv4_results_append'}),
    # the baseline JPEG decoder, EXIF orientation in it, the Huffman scan decode on the device and its self-synchronising
    # chunk form
    'jpeg': Feature({'yv4_jpeg_parse', 'yv4_jpeg_entropy_decode', 'yv4_jpeg_layout', 'yv4_jpeg_reconstruct'}),
    'jpeg_orientation': Feature({'yv4_jpeg_layout_oriented'}),
    'jpeg_entropy': Feature({'yv4_jpeg_scan_prepare', 'yv4_jpeg_entropy_workgroups', 'yv4_jpeg_entropy_decode_segments',
                             'yv4_jpeg_entropy_decode_device', 'yv4_jpeg_entropy_strerror'}),
    'jpeg_sync': Feature({'yv4_jpeg_chunks_build', 'yv4_jpeg_entropy_decode_sync', 'yv4_jpeg_entropy_decode_device_sync'},
                         ('jpeg_entropy',)),
    # the baseline JPEG encoder
    'jpeg_encode': Feature({'yv4_jpeg_encode_layout', 'yv4_jpeg_encode_validate', 'yv4_jpeg_encode_header',
                            'yv4_jpeg_encode_host', 'yv4_jpeg_encode_coefficients', 'yv4_jpeg_encode_scan'}),
    # drawing detections onto images; with flags (boxes without a score)
    'draw': Feature({'yv4_draw_layout', 'yv4_draw_boxes', 'yv4_draw_boxes_host'}),
    'draw_ex': Feature({'yv4_draw_boxes_ex', 'yv4_draw_boxes_host_ex'}, ('draw',)),
    # the per-image mAP
    'map_image': Feature({'yv4_map_image_ap_work', 'yv4_map_image_ap', 'yv4_map_image_mean'}),
    # the proposal recall
    'recall': Feature({'yv4_recall_work', 'yv4_recall_match'}),
    # the fused YOLOv3 loss
    'v3_loss': Feature({'yv4_yolov3_loss_fwd', 'yv4_yolov3_loss_bwd'}, abi=8),
}
DRAW_NO_SCORE = 1          # YV4_DRAW_NO_SCORE
RECALL_MAX_NUMS, RECALL_MAX_THRS, RECALL_LDS_BOXES = 16, 256, 1280      # csrc/recall.hip: kRcMaxNums, kRcMaxThrs, kRcLdsBoxes
#: ``YV4_JPEG_MIN_CHUNK_BYTES`` / ``YV4_JPEG_MAX_CHUNK_BYTES`` / ``YV4_JPEG_MAX_ROUNDS`` (include/yv4.h)
JPEG_MIN_CHUNK_BYTES, JPEG_MAX_CHUNK_BYTES, JPEG_MAX_ROUNDS = 4, 1 << 20, 4096
#: ``YV4_RESULTS_MAX_PER_IMG`` (include/yv4.h): the labels of one image that yv4_results_append holds in LDS
RESULTS_MAX_PER_IMG = 4096
#: ``YV4_COCO_ERROR_LDS_PAIRS`` / ``YV4_COCO_ERROR_LDS_GTS`` (an enum of include/yv4.h): the IoU block (doubles) and the ground truths
#: of an image up to which a problem of yv4_coco_error_match stays in LDS; beyond either it takes the workspace
COCO_ERROR_LDS_PAIRS, COCO_ERROR_LDS_GTS = 9216, 512

_lock = threading.Lock()
_lib = None
_has = None                # {feature: present in the bound library}, from _bind


def build(verbose=False, measure=False):
    """Compile the HIP sources for gfx950 into ``lib/libyv4_hip.so`` (in-tree).  ``measure``: the -DYV4_MEASURE build,
    ``lib_alt/libyv4_hip_measure.so``, instead -- the only library in which the kernel forms behind the measurement
    switches can be reached (tests/test_gpu_bn_exact.py runs them in child processes)."""
    cmd = ['make', '-C', CSRC_DIR, '-j4'] + (['measure'] if measure else [])
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True)
    if verbose or res.returncode != 0:
        print(res.stdout)
    if res.returncode != 0:
        raise RuntimeError('building libyv4_hip.so failed (see output above)')
    return os.path.join(os.path.dirname(LIB_DIR), 'lib_alt', 'libyv4_hip_measure.so') if measure else LIB_PATH


def lib():
    """Load (once) and return the bound library.  No fallback: raises if absent."""
    global _lib, _has
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f'{LIB_PATH} is missing: the HIP extension has not been built. '
                'Run `python -c "import __graft_entry__ as g; g.build()"` (or '
                f'`make -C {CSRC_DIR}`). There is no CPU fallback for this path.')
        handle = C.CDLL(LIB_PATH)
        present = _bind(handle)
        got = handle.yv4_abi_version()
        if got != ABI_VERSION and not (os.environ.get('YV4_LIB_PATH') and os.environ.get('YV4_LIB_ABI_ANY') == '1'
                                       and got == ABI_VERSION - 1):
            # (YV4_LIB_ABI_ANY=1 with YV4_LIB_PATH: same-box A/B against the previous ABI's build -- ABI 8 only APPENDED
            # the YOLOv3 loss entry points, which are left unbound for an ABI-7 library: FEATURES['v3_loss'])
            raise RuntimeError(f'libyv4_hip.so ABI {got} != binding ABI {ABI_VERSION}; rebuild')
        form = os.environ.get('YV4_NMS_IOU_FORM', '').lower()
        if form in ('mul', '1', 'product', 'cuda'):
            handle.yv4_nms_set_iou_form(NMS_IOU_MUL)      # mmcv's CUDA-kernel predicate instead of its CPU kernel's
        _has, _lib = present, handle
    return _lib


def _bind(handle):
    """Give every entry point of ``handle`` its prototype from ``SIGNATURES`` by the rule of ``FEATURES`` (a symbol of
    no feature that is missing: ``AttributeError``) -> ``{feature: present}``, what ``has`` answers from."""
    handle.yv4_abi_version.restype, handle.yv4_abi_version.argtypes = SIGNATURES['yv4_abi_version']
    abi = handle.yv4_abi_version()
    owner = {s: ft for ft in FEATURES.values() for s in ft.symbols}
    for name, (res, args) in SIGNATURES.items():
        ft = owner.get(name)
        if ft is not None and (abi < ft.abi if ft.abi else not hasattr(handle, name)):
            continue                # an optional symbol that this library does not have
        fn = getattr(handle, name)  # AttributeError if a symbol is missing
        fn.restype = res
        fn.argtypes = args
    own = {f: abi >= ft.abi if ft.abi else all(hasattr(handle, s) for s in ft.symbols) for f, ft in FEATURES.items()}
    return {f: own[f] and all(own[r] for r in ft.requires) for f, ft in FEATURES.items()}


def has(feature):
    """The loaded library exports every entry point of ``FEATURES[feature]`` and of the features it requires."""
    lib()
    return _has[feature]


def require(feature, what=None):
    """``RuntimeError`` naming the missing entry points unless ``has(feature)``.  ``what``: the caller, or the argument as
    the user wrote it, that asks for the feature."""
    if has(feature):
        return
    names = [s for f in (feature,) + tuple(FEATURES[feature].requires) for s in sorted(FEATURES[f].symbols)]
    missing = ' / '.join([s for s in names if not hasattr(_lib, s)] or names)      # (all: left unbound by the ABI rule)
    if what is None:
        raise RuntimeError(f'the loaded libyv4_hip.so has no {missing}: rebuild it')
    raise RuntimeError(f'{what} needs {missing}, which the loaded libyv4_hip.so does not export (there is no fallback): '
                       'rebuild it')


class Yv4Error(RuntimeError):
    """A C-ABI call returned a non-zero status."""


def check(status, what):
    if status != 0:
        msg = lib().yv4_last_error().decode('utf-8', 'replace')
        raise Yv4Error(f'{what} failed with status {status}: {msg}')
