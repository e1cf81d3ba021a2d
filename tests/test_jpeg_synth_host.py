"""The JPEG decoders on streams that no encoder writes, without a GPU.  ``tests/_jpeg_synth.py`` writes the files from
chosen coefficients and chosen Huffman tables, so what a decoder has to return is known without a decoder: the restatement
``_jpeg_ref.py`` is held to the writer, then the library's three entropy paths -- the host oracle
(``yv4_jpeg_entropy_decode``), the segment core and the chunk core on the CPU -- at every chunk size, and libjpeg-turbo's
pixels (``tests/golden/jpeg_synth.npz``) to the restatement's.  A census, taken with the restatement's bit reader, states
what each case reaches and what the 84 encoder-made fixture files never do (DESIGN 19.4 holds the table it prints)."""
import ctypes

import numpy as np
import pytest

import mmdet_yolov4_amd as pkg
from mmdet_yolov4_amd import image_io
import _jpeg_ref as R
import _jpeg_synth as S
from test_jpeg_host import _same_info

L = pkg._lib
MIN = L.JPEG_MIN_CHUNK_BYTES
CHUNK_BYTES = (4, 5, 7, 16, 64, 256)
MESSAGE = {S.ERR_DC_CATEGORY: 'DC magnitude category', S.ERR_INDEX: 'coefficient index', S.ERR_CODE: 'code that is in no Huffman table'}


@pytest.fixture(scope='module')
def synth():
    """name -> (file bytes, the writer's coefficients): written once"""
    return {name: S.make(name)[:2] for name in S.CASES}


@pytest.fixture(scope='module')
def invalid():
    return {name: (S.make(name)[0], code) for name, (_, code) in S.INVALID.items()}


# ---- the census: the restatement's bit reader, instrumented here ------------------------------------------------------

class _Reader(R._Bits):
    """``_jpeg_ref._Bits`` that notes every symbol (table, symbol, first bit) and where every magnitude field ends.  Bit
    positions count raw file bytes, stuffed zeros included."""
    made = []

    def __init__(self, d, pos):
        super().__init__(d, pos)
        self.at, self.events = pos, []
        _Reader.made.append(self)

    def where(self):
        return self.pos * 8 if self.left == 0 else self.at * 8 + 8 - self.left

    def bit(self):
        if self.left == 0:
            self.at = self.pos
        return super().bit()

    def symbol(self, table):
        start = self.where()
        sym = super().symbol(table)
        self.events.append([id(table), sym, start, self.where()])
        return sym

    def value(self, s):
        v = super().value(s)
        self.events[-1][3] = self.where()
        self.events[-1].append(v)
        return v


def census(data):
    """What a file's scan reaches, from the restatement's decode of it."""
    plain, R._Bits, _Reader.made = R._Bits, _Reader, []
    try:
        info, coef = R.entropy_decode(data)
    finally:
        R._Bits = plain
    events = _Reader.made[0].events
    d = bytes(data)
    which, length = {}, {}
    for cls, tables in ((0, info['dc']), (1, info['ac'])):
        for slot, t in tables.items():
            which[id(t)] = (cls, slot)
            length[id(t)] = {sym: n for (n, _), sym in t.items()}
    sampling = {(1, 1, 1): 'gray', (3, 1, 1): '444', (3, 2, 1): '422', (3, 2, 2): '420'}[(info['ncomp'], info['hs'][0], info['vs'][0])]
    lay = S.Layout(info['width'], info['height'], sampling)
    c = dict(lengths=({}, {}), dc_cat=0, ac_size=0, zrl=0, zrl_eob=0, no_eob=0, blocks=0, raw_max=0, dc_extreme=0,
             starts=set(), codes=set(), info=info, coef=coef)
    block, ordinal, run = [], -1, [0] * lay.ncomp
    ri = info['restart_interval'] * lay.bpm

    def close():
        if block:
            c['no_eob'] += block[-1] != S.EOB
            c['zrl_eob'] += len(block) > 1 and block[-1] == S.EOB and block[-2] == S.ZRL
    for e in events:
        cls, slot = which[e[0]]
        n = length[e[0]][e[1]]
        c['lengths'][cls][n] = c['lengths'][cls].get(n, 0) + 1
        c['codes'].add((cls, slot, n, next(code for (m, code), s in (info['ac'] if cls else info['dc'])[slot].items()
                                           if m == n and s == e[1])))
        c['starts'].add(e[2] // 8)
        c['raw_max'] = max(c['raw_max'], (e[3] - 1) // 8 - e[2] // 8 + 1)
        if cls == 0:
            close()
            block, ordinal = [], ordinal + 1
            if ri and ordinal % ri == 0:
                run = [0] * lay.ncomp
            c['dc_cat'] = max(c['dc_cat'], e[1])
            run[lay.comp[ordinal]] += e[4] if len(e) > 4 else 0
            c['dc_extreme'] = max(c['dc_extreme'], abs(run[lay.comp[ordinal]]))
        else:
            block.append(e[1])
            c['zrl'] += e[1] == S.ZRL
            if e[1] & 15:
                c['ac_size'] = max(c['ac_size'], e[1] & 15)
    close()
    c['blocks'] = ordinal + 1
    scan = info['scan_offset']
    c['scan_bytes'] = len(d) - 2 - scan
    c['stuffed'] = sum(d[i] == 0xFF and d[i + 1] == 0 for i in range(scan, len(d) - 1))
    c['slots'] = (sorted(set(info['td'])), sorted(set(info['ta'])), sorted(set(info['tq'])))
    c['tables'] = len({(0, s) for s in info['td']} | {(1, s) for s in info['ta']})
    c['definitions'] = _dht_definitions(d, scan)
    c['sof1'] = any(d[i] == 0xFF and d[i + 1] == 0xC1 for i in _markers(d, scan))
    return c


def _markers(d, scan):
    """offsets of the header segments' markers in front of the scan"""
    pos, out = 2, []
    while pos < scan:
        out.append(pos)
        pos += 2 + ((d[pos + 2] << 8) | d[pos + 3])
    return out


def _dht_definitions(d, scan):
    """(class, slot) of every table definition of the headers, in file order; the number of DHT segments"""
    defs, segments = [], 0
    for i in _markers(d, scan):
        if d[i + 1] == 0xC4:
            segments += 1
            seg = d[i + 4:i + 2 + ((d[i + 2] << 8) | d[i + 3])]
            while seg:
                defs.append((seg[0] >> 4, seg[0] & 15))
                seg = seg[17 + sum(seg[1:17]):]
    return defs, segments


@pytest.fixture(scope='module')
def synth_census(synth):
    return {name: census(data) for name, (data, _) in synth.items()}


def _row(title, cs):
    """One line of the census table over the files ``cs``."""
    def lens(cls):
        used = sorted({n for c in cs for n in c['lengths'][cls]})
        return ','.join(map(str, used))
    slots = [sorted({s for c in cs for s in c['slots'][k]}) for k in range(3)]
    twice = sum(len(set(c['definitions'][0])) < len(c['definitions'][0]) for c in cs)
    return (f'{title:<18} files {len(cs):3d} | DC lengths {lens(0)} | AC lengths {lens(1)} | DC category <= {max(c["dc_cat"] for c in cs)}'
            f' | AC size <= {max(c["ac_size"] for c in cs)} | ZRL {sum(c["zrl"] for c in cs)} | ZRL before EOB '
            f'{sum(c["zrl_eob"] for c in cs)} | blocks without EOB {sum(c["no_eob"] for c in cs)} | stuffed pairs '
            f'{sum(c["stuffed"] for c in cs)} | longest symbol {max(c["raw_max"] for c in cs)} raw bytes | slots td {slots[0]} '
            f'ta {slots[1]} tq {slots[2]} | tables per file <= {max(c["tables"] for c in cs)} | SOF1 {sum(c["sof1"] for c in cs)}'
            f' | a table defined twice {twice} | |running DC| <= {max(c["dc_extreme"] for c in cs)}')


# ---- the writer ---------------------------------------------------------------------------------------------------------

def test_the_two_zigzag_literals_are_equal():
    assert list(S.ZIGZAG) == R.ZIGZAG.tolist() and sorted(S.ZIGZAG) == list(range(64))


def test_table_helpers_give_canonical_codes():
    counts, vals, codes = S.canonical(S.unary(range(16)))
    assert counts == [1] * 16 and vals == list(range(16))
    assert all(codes[i] == (i + 1, (1 << (i + 1)) - 2) for i in range(16))      # 0, 10, 110, ...: ones ending in 0
    t = S.flat(list(range(256)), 8)
    assert sorted(t.values()) == [8] * 255 + [9] and S.canonical(t)[2][255] == (9, 510)
    assert set(S.flat(list(range(12)), 4).values()) == {4}
    assert S.canonical(S.at_length(0x01, 16, S.AC_OTHERS))[2][0x01] == (16, 0xFFFE)
    assert S.canonical(S.at_length(0x01, 1, S.AC_OTHERS))[2] == {0x01: (1, 0), S.EOB: (2, 2)}
    for bad in ({0: 1, 1: 1}, {0: 1, 1: 2, 2: 2}, {0: 16, 1: 0}):      # all ones, over-full, a zero length
        with pytest.raises(AssertionError):
            S.canonical(bad)


def test_case_list_holds_what_the_design_names(synth):
    want = {f'len_{c}_{n}' for c in ('dc', 'ac') for n in range(1, 17)} | {'deep_' + s for s in S.SAMPLINGS} | {
        'look_9_10', 'flat8_444', 'single_gray', 'sym256_ac', 'slots23_444', 'redefined_420', 'dht_split', 'dht_joined',
        'dc_cat11', 'dc_wrap', 'dc_wrap_rst', 'ac_wide', 'full_block', 'only_k63', 'zrl_eob', 'runs', 'ones_dense_plain',
        'ones_dense_rst', 'wide_ones', 'basis_q1', 'basis_q255'} | {f'padding_loud_{s}_{z}' for s in ('422', '420')
                                                                    for z in ('9x7', '17x33')}
    assert want <= set(synth) and sum(n.startswith('rst_') for n in synth) >= 4
    assert set(S.INVALID) == {'bad_dc_category', 'bad_index', 'bad_code'}
    for name, (data, _) in synth.items():
        info = R.parse(data)
        big = name.startswith('basis_') or name == 'rst_1_gray'
        assert info['width'] * info['height'] <= (64 * 128 if big else 48 * 64), name


def test_restatement_returns_what_the_writer_wrote(synth):
    for name, (data, want) in synth.items():
        info, got = R.entropy_decode(data)
        assert got.dtype == np.int16 and got.shape == want.shape, name
        np.testing.assert_array_equal(got, want, err_msg=name)


def test_dc_predictor_wraps_to_int16_in_the_restatement(synth, synth_census):
    for name in ('dc_wrap', 'dc_wrap_rst'):
        data, want = synth[name]
        assert synth_census[name]['dc_extreme'] > 32767, name      # the unwrapped running sum leaves int16 ...
        dc = want.reshape(-1, 64)[:, 0].astype(np.int64)
        assert dc.min() < -16384 and dc.max() > 16384             # ... and the stored terms come back on the other side
        np.testing.assert_array_equal(R.entropy_decode(data)[1], want, err_msg=name)
    assert R.parse(synth['dc_wrap_rst'][0])['restart_interval'] == 22 and R.parse(synth['dc_wrap'][0])['restart_interval'] == 0


# ---- the library against the writer ---------------------------------------------------------------------------------------

def test_library_parse_equals_the_restatements(synth):
    for name, (data, _) in synth.items():
        _same_info(image_io.jpeg_parse(data), R.parse(data))


def test_host_oracle_and_segment_core_return_what_the_writer_wrote(synth):
    for name, (data, want) in synth.items():
        np.testing.assert_array_equal(image_io.jpeg_entropy_decode(data)[1], want, err_msg=name)
        _, coef, status = image_io.jpeg_entropy_decode_segments([data])
        assert status[0] == 0, name
        np.testing.assert_array_equal(coef, want, err_msg=name)
    names = list(synth)                              # and as one batch: mixed tables, image after image
    t, coef, status = image_io.jpeg_entropy_decode_segments([synth[n][0] for n in names])
    assert not status.any()
    for n, sc in zip(names, t.scans):
        np.testing.assert_array_equal(coef[sc.coef_off:sc.coef_off + sc.ncoef], synth[n][1], err_msg=n)


@pytest.mark.parametrize('chunk_bytes', CHUNK_BYTES)
def test_chunk_core_returns_what_the_writer_wrote_with_nothing_undecided(synth, chunk_bytes):
    for name, (data, want) in synth.items():
        _, _, _, coef, status, undecided, rounds = image_io.jpeg_entropy_decode_sync([data], chunk_bytes, L.JPEG_MAX_ROUNDS)
        assert status[0] == 0 and undecided[0] == 0 and rounds < L.JPEG_MAX_ROUNDS, (name, rounds)
        np.testing.assert_array_equal(coef, want, err_msg=name)


def test_chunk_core_without_rounds_takes_the_second_decode(synth):
    for name in ('wide_ones', 'ones_dense_plain', 'deep_420', 'slots23_444', 'dc_wrap'):
        data, want = synth[name]
        _, ch, _, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([data], MIN, 0)
        assert status[0] == 0 and ch.nchunk > 1, name
        np.testing.assert_array_equal(coef, want, err_msg=name)


def test_six_tables_and_the_last_definition_are_packed(synth):
    t = image_io.ScanTables([synth['slots23_444'][0]])
    sc = t.scans[0]
    assert sc.nhuff == 6 and sorted(list(sc.td)[:3] + list(sc.ta)[:3]) == list(range(6))
    for name in ('redefined_420', 'redefined_joined_420'):
        a, b = image_io.ScanTables([synth[name][0]]), image_io.ScanTables([synth['dht_joined'][0]])
        assert a.scans[0].nhuff == b.scans[0].nhuff == 4
        n = 4 * ctypes.sizeof(L.JpegHuff)
        assert bytes(a.huff)[:n] == bytes(b.huff)[:n], name


def test_invalid_files_end_with_their_error_in_every_path(invalid):
    for name, (data, code) in invalid.items():
        with pytest.raises(R.Invalid):
            R.entropy_decode(data)
        with pytest.raises(ValueError, match=MESSAGE[code]):
            image_io.jpeg_entropy_decode(data)
        assert image_io.jpeg_entropy_decode_segments([data])[2][0] == code, name
        for cb in CHUNK_BYTES:
            r = image_io.jpeg_entropy_decode_sync([data], cb, L.JPEG_MAX_ROUNDS)
            assert r[4][0] == code, (name, cb)


# ---- the census -------------------------------------------------------------------------------------------------------

def test_each_case_reaches_what_its_name_claims(synth, synth_census):
    cs = synth_census
    for s in S.SAMPLINGS:
        c = cs['deep_' + s]
        assert set(c['lengths'][0]) | set(c['lengths'][1]) == set(range(1, 17)) and set(c['lengths'][1]) == set(range(1, 17)), s
        if s != 'gray':
            assert set(c['lengths'][0]) == set(range(1, 17))
    for n in range(1, 17):
        for cls, kind in ((0, 'dc'), (1, 'ac')):
            used = cs[f'len_{kind}_{n}']['lengths'][cls]
            assert 2 * used.get(n, 0) >= sum(used.values()) > 0, (kind, n)
    c = cs['look_9_10']
    last9 = max(code for cls, _, n, code in c['codes'] if cls == 1 and n == 9)
    assert (1, 0, 10, (last9 + 1) << 1) in c['codes'] and (1, 0, 9, last9) in c['codes'] and last9 == 359
    assert set(cs['flat8_444']['lengths'][0]) == {8, 9} and set(cs['flat8_444']['lengths'][1]) == {8, 9}
    assert cs['single_gray']['lengths'] == ({1: 15}, {1: 15}) and cs['single_gray']['dc_cat'] == 0
    assert len(R.parse(synth['sym256_ac'][0])['ac'][0]) == 256
    c = cs['slots23_444']
    assert c['tables'] == 6 and c['slots'] == ([0, 2, 3], [1, 2, 3], [1, 2, 3]) and c['sof1']
    assert len({tuple(sorted(t.items())) for t in list(c['info']['dc'].values()) + list(c['info']['ac'].values())}) == 6
    assert len({c['info']['quant'][q].tobytes() for q in (1, 2, 3)}) == 3
    for name, segments in (('redefined_420', 7), ('redefined_joined_420', 1)):
        defs = cs[name]['definitions']
        assert defs[1] == segments and len(defs[0]) == 7 and len(set(defs[0])) == 4, name
    assert cs['dht_split']['definitions'] == ([(0, 0), (0, 1), (1, 0), (1, 1)], 4) and cs['dht_joined']['definitions'][1] == 1
    assert synth['dht_split'][1].tobytes() == synth['dht_joined'][1].tobytes() == synth['redefined_420'][1].tobytes()
    assert cs['dc_cat11']['dc_cat'] == 11 and cs['dc_cat11']['lengths'][0].get(12, 0) > 0
    assert cs['ac_wide']['ac_size'] == 15 and cs['ac_wide']['lengths'][1].get(16, 0) >= 15 and cs['ac_wide']['raw_max'] >= 4
    sizes = {abs(int(v)).bit_length() for v in synth['ac_wide'][1].reshape(-1, 64)[:, 1:].ravel()}
    assert {11, 12, 13, 14, 15} <= sizes
    assert cs['full_block']['no_eob'] == cs['full_block']['blocks'] == 6
    assert cs['only_k63']['no_eob'] == 6 and cs['only_k63']['zrl'] == 18
    assert cs['zrl_eob']['zrl_eob'] > 0 and cs['zrl_eob']['zrl'] >= 2 * cs['zrl_eob']['zrl_eob']
    runs = {(int(k) >> 4, int(k) & 15) for k in R.parse(synth['runs'][0])['ac'][0].values()}
    assert {(r, s) for r in range(16) for s in (1, 10)} <= runs and cs['runs']['ac_size'] == 10
    seen = set()
    for blk in synth['runs'][1].reshape(-1, 64):
        zz, run = blk[list(S.ZIGZAG)], 0
        for v in zz[1:]:
            if v == 0:
                run += 1
            else:
                seen.add((run, abs(int(v)).bit_length()))
                run = 0
    assert {(r, s) for r in range(16) for s in (1, 10)} <= seen
    for name in ('ones_dense_plain', 'ones_dense_rst'):
        assert 8 * cs[name]['stuffed'] >= cs[name]['scan_bytes'], (name, cs[name]['stuffed'], cs[name]['scan_bytes'])
    assert R.parse(synth['ones_dense_rst'][0])['restart_interval'] == 1
    for name in [n for n in synth if n.startswith('padding_loud_')]:
        info, coef = cs[name]['info'], synth[name][1].reshape(-1, 64)
        pad = S.loud_terms(S.Layout(info['width'], info['height'], name.split('_')[2]))
        assert pad.any() and (np.abs(coef[pad][:, 0]) == 1000).all() and (np.abs(coef[pad][:, 1:]).max(1) == 200).all()
        assert np.abs(coef[~pad][:, 0]).max() < 1000, name      # no visible block carries a loud block's terms
    for name in ('basis_q1', 'basis_q255'):
        coef = synth[name][1].reshape(128, 64)
        assert all(np.count_nonzero(coef[b]) == 1 and coef[b, b // 2] == (-1) ** b * coef[0, 0] for b in range(128))
    assert int(synth['basis_q1'][1][0]) * 1 == int(synth['basis_q255'][1][0]) * 255 == 2040


def test_wide_ones_leaves_chunks_without_a_symbol_start(synth, synth_census):
    data, _ = synth['wide_ones']
    c = synth_census['wide_ones']
    begin, end = c['info']['scan_offset'], len(data) - 2
    assert c['raw_max'] > MIN and c['stuffed'] > 200
    chunks = range(begin, end, MIN)
    assert sum(not any(b in c['starts'] for b in range(at, min(at + MIN, end))) for at in chunks) > 0
    assert sum(data[at] == 0 and data[at - 1] == 0xFF for at in chunks[1:]) > 0
    # the chunk tables see the same: an entry that lies beyond its whole chunk, an entry moved off the stuffed zero
    t, ch, entries, coef, status, undecided, _ = image_io.jpeg_entropy_decode_sync([data], MIN, L.JPEG_MAX_ROUNDS)
    assert ch.nchunk == len(chunks) > 128 and status[0] == 0 and undecided[0] == 0
    beyond = [g for g in range(ch.nchunk - 1) if entries[g].entry >> 19 >= begin + (g + 1) * MIN]
    assert beyond and all(entries[g].nblk == 0 for g in beyond)
    assert all(data[entries[g].entry >> 19] != 0 or data[(entries[g].entry >> 19) - 1] != 0xFF for g in range(1, ch.nchunk))
    # a previous chunk's exit beyond the whole next chunk: the entry of chunk g + 1 lies behind chunk g + 1
    assert any(entries[g + 1].entry >> 19 >= begin + (g + 2) * MIN for g in range(ch.nchunk - 2))


def test_census_of_the_encoder_made_fixtures_against_the_synthetic_ones(golden, synth_census):
    """Prints the table of DESIGN 19.4 and asserts what it is quoted for: what no encoder-made file reaches."""
    a, b = golden('jpeg'), golden('jpeg_entropy')
    old = [census(g['jpg_' + str(n)].tobytes()) for g in (a, b) for n in g['names']]
    new = list(synth_census.values())
    assert len(old) == 84
    print()
    print(_row('jpeg + entropy', old))
    print(_row('jpeg_synth', new))
    used = [{n for c in old for n in c['lengths'][cls]} for cls in (0, 1)]
    assert max(used[0]) == 10 and used[1] == set(range(1, 17)) - {13}      # the slow path's lengths, but for one, by AC only
    assert max(c['dc_cat'] for c in old) == 10 and max(c['ac_size'] for c in old) == 9
    assert all(set(c['slots'][k]) <= {0, 1} for c in old for k in range(3)) and max(c['tables'] for c in old) <= 4
    assert not any(c['sof1'] for c in old) and sum(c['zrl_eob'] for c in old) == 0
    assert all(len(set(c['definitions'][0])) == len(c['definitions'][0]) for c in old)
    assert max(c['raw_max'] for c in old) == 6 < max(c['raw_max'] for c in new) and max(c['dc_extreme'] for c in old) <= 2047
    assert sum(c['no_eob'] for c in old) > 0      # the quality-100 noise files do end blocks at k = 63
    assert {n for c in new for n in c['lengths'][0]} == {n for c in new for n in c['lengths'][1]} == set(range(1, 17))
    assert max(c['dc_cat'] for c in new) == 11 and max(c['ac_size'] for c in new) == 15


# ---- the fixture --------------------------------------------------------------------------------------------------------

def test_writer_reproduces_the_fixture_byte_for_byte(golden, synth, invalid):
    g = golden('jpeg_synth')
    assert [str(n) for n in g['names']] == list(synth) and [str(n) for n in g['invalid']] == list(invalid)
    for name in synth:
        assert g['jpg_' + name].tobytes() == synth[name][0], name
    for name in invalid:
        assert g['jpg_' + name].tobytes() == invalid[name][0], name


def test_restatement_equals_libjpeg_turbo_where_the_fixture_has_pixels(golden, synth):
    g = golden('jpeg_synth')
    unpinned = {str(n) for n in g['unpinned_pixels']}
    assert unpinned == {'dc_wrap', 'dc_wrap_rst', 'ac_wide', 'runs', 'ones_dense_plain', 'ones_dense_rst', 'wide_ones'}
    for name, (data, _) in synth.items():
        assert ('rgb_' + name in g.files) == (name not in unpinned), name
        if name not in unpinned:
            np.testing.assert_array_equal(R.decode(data, 'rgb'), g['rgb_' + name], err_msg=name)
    # the padding is loud enough to show: a decode that took the padded chroma samples for real ones differs
    # (at an even size only: an odd size's last column and row interpolate towards the inside)
    for name in ('padding_loud_420_10x6', 'padding_loud_422_10x6'):
        info, coef = R.entropy_decode(synth[name][0])
        wrong = dict(info, width=info['blocks_w'][0] * 8, height=info['blocks_h'][0] * 8)
        got = R.reconstruct(wrong, coef, 'rgb')[:info['height'], :info['width']]
        assert (got != g['rgb_' + name]).any(), name
