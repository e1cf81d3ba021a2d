"""``tools/tencent_image_split.py`` on the GPU: every tile file equals ``imencode`` of a contiguous copy of the same crop,
byte for byte, and the tile names and label files equal what the reference's tool writes (tests/golden/custom_sets.npz,
``split/...``).  Sources of 100 x 70, 64 x 48 and 40 x 30 with tile (64, 48) and overlap (16, 16): byte offsets of 108 into
a 300-byte pitch (no 16-byte alignment anywhere), a clamped last tile, a whole-picture tile and a short tile."""
import importlib.util
import os

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ('big', 'fit', 'small')


def _tool():
    spec = importlib.util.spec_from_file_location('tool_tencent_image_split', os.path.join(ROOT, 'tools', 'tencent_image_split.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize('batch', [16, 1])
def test_tiles_equal_imencode_of_the_crop_and_the_reference_labels(golden, tmp_path, gpu_device, batch):
    g = golden('custom_sets')
    src, dst = tmp_path / 'in', tmp_path / 'out'
    os.makedirs(src / 'img')
    os.makedirs(src / 'label')
    for name in SOURCES:
        with open(src / 'img' / f'{name}.jpg', 'wb') as f:
            f.write(g[f'jpg/split_{name}'].tobytes())
        with open(src / 'label' / f'{name}.circle', 'w') as f:
            f.writelines(g[f'split/{name}/rows'].tolist())
    tool = _tool().TencentImageSplitTool(str(src), str(dst), tile_overlap=(16, 16), tile_shape=(64, 48), batch=batch,
                                         device=gpu_device)
    assert tool.image_ids == sorted(SOURCES)
    written = tool.split()
    want_names = [n for name in sorted(SOURCES) for n in g[f'split/{name}/tiles'].tolist()]
    assert written == want_names and len(written) == 6
    assert sorted(os.listdir(dst / 'img')) == sorted(n + '.jpg' for n in want_names)
    assert sorted(os.listdir(dst / 'label')) == sorted(n + '.circle' for n in want_names)
    for name in SOURCES:
        picture = pkg.imread(str(src / 'img' / f'{name}.jpg'), device=gpu_device, orientation=True)
        for tile, (w_off, h_off), (th, tw) in zip(g[f'split/{name}/tiles'].tolist(), g[f'split/{name}/offsets'].tolist(),
                                                  g[f'split/{name}/shapes'].tolist()):
            with open(dst / 'label' / f'{tile}.circle') as f:
                assert f.read() == str(g[f'split/{name}/label/{tile}'])
            crop = picture[h_off:h_off + 48, w_off:w_off + 64].contiguous()
            assert tuple(crop.shape) == (th, tw, 3)
            with open(dst / 'img' / f'{tile}.jpg', 'rb') as f:
                data = f.read()
            assert data == pkg.imencode(crop), tile
            assert tuple(pkg.imdecode(data, device=gpu_device).shape) == (th, tw, 3)
    assert np.asarray(g['split/big/offsets']).tolist()[1] == [36, 0]                  # 3 * 36 = 108 bytes into the row
