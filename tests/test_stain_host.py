"""CPU tests of the stain passes' specification and surroundings: include/hdyolo_stain.h and its binding through _ext.PIXEL_EXTENSIONS, every
argument check of the four entry points (reached with fake pointers: nothing launches), the arithmetic bounds of the tables over all 256
values, the numpy restatement (tests/stain_ref.py) and the estimator of hd_yolo_amd/stain.py on synthetic slides of known stains against the
float64 ideal, the percentile rule, the flags, the tables, the recolouring against the real-valued ideal, and the matrix hook of
texture.texture_table."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

import stain_ref as ref
import texture_ref
from hd_yolo_amd import _header, _lib, build, synth
from hd_yolo_amd import stain as hstain
from hd_yolo_amd import texture as htexture

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAKE = 0x10000      # an aligned non-NULL "device pointer": every call below must fail validation before anything dereferences or launches
M0 = htexture.stain_matrix().numpy()


def _rot(v, axis, deg):
    """v turned by deg degrees about axis (Rodrigues)"""
    v, k, t = np.asarray(v, float), np.asarray(axis, float) / np.linalg.norm(axis), math.radians(deg)
    return v * math.cos(t) + np.cross(k, v) * math.sin(t) + k * (k @ v) * (1 - math.cos(t))


# the Ruifrok vectors and two pairs turned by 5 to 10 degrees, each with the 99th-percentile concentrations its slide is drawn with
PAIRS = [((M0[0], M0[1]), (0.8558, 0.4477)),
         ((_rot(M0[0], (0, 0, 1), 7), _rot(M0[1], (1, 0, 0), -6)), (0.9, 0.5)),
         ((_rot(M0[0], (0, 1, 0), -8), _rot(M0[1], (0, 0, 1), -5)), (1.1, 0.4))]


def _matrix(h, e):
    r = np.cross(h, e)
    return np.stack([h, e, r / np.linalg.norm(r)])


# ---- the extension header and its binding, through the built library ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    from hd_yolo_amd import _ext
    return _ext.load()


def test_stain_header_parses_and_is_bound_in_the_pixel_table(lib):
    from hd_yolo_amd import _ext
    path = os.path.join(ROOT, 'include', 'hdyolo_stain.h')
    assert _header.PIXEL_EXTENSION_NAMES == ('stain',) and list(_ext.PIXEL_EXTENSIONS) == ['stain']
    ext = _ext.PIXEL_EXTENSIONS['stain']
    assert ext.header == path == _header.extension_header('stain')
    hdr = _header.read(path)
    assert sorted(hdr.functions) == ['hdy_stain_angles_u8', 'hdy_stain_apply_u8', 'hdy_stain_levels_u8', 'hdy_stain_moments_u8',
                                     'hdy_stain_revision'] and not hdr.structs
    assert hdr.constants == {'HDY_STAIN_REVISION': 1, 'HDY_STAIN_OD_SHIFT': 10, 'HDY_STAIN_ANGLE_SHIFT': 4, 'HDY_STAIN_SHIFT': 16,
                             'HDY_STAIN_MAX_BINS': 1024, 'HDY_STAIN_MAX_TONE': 8192, 'HDY_STAIN_MAX_SIDE': 1 << 29, 'HDY_STAIN_MAX_BLOCKS': 1024}
    vp, ll, i = ctypes.c_void_p, ctypes.c_longlong, ctypes.c_int
    common = [vp, ll, i, i, i, i, i, i, i]
    assert hdr.functions['hdy_stain_moments_u8'] == (i, common + [i, i, vp, ll, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_stain_angles_u8'] == (i, common + [i, i, vp, ll, i, vp, ll, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_stain_levels_u8'] == (i, common + [i, i, vp, ll, i, vp, ll, vp, ll, vp])
    assert hdr.functions['hdy_stain_apply_u8'] == (i, common + [vp, ll, i, vp, ll, vp, ll, i, vp])
    assert [p[0] for p in hdr.params['hdy_stain_angles_u8']][:11] == ['slide', 'pitch_bytes', 'pixel_bytes', 'H', 'W', 'x0', 'y0', 'w', 'h', 'step',
                                                                      'background']
    for name, (res, args) in hdr.functions.items():
        fn = getattr(lib, name)                                            # exported by the built library ...
        assert fn.restype is res and list(fn.argtypes) == args, name      # ... and bound by _ext.load()
        assert name not in _lib.SIGNATURES and name not in _ext.SIGNATURES
        assert _ext.PIXEL_SIGNATURES[name] == (res, args) and _ext.PIXEL_PARAMS[name] == hdr.params[name]
    assert (ext.functions, ext.params, ext.constants) == (hdr.functions, hdr.params, hdr.constants)
    assert (ext.revision_fn, ext.revision_macro) == ('hdy_stain_revision', 'HDY_STAIN_REVISION')
    assert lib.hdy_stain_revision() == ext.revision == 1
    assert _ext.PIXEL_CONSTANTS == hdr.constants
    assert (hstain.OD_SHIFT, hstain.ANGLE_SHIFT, hstain.SHIFT, hstain.MAX_BINS, hstain.MAX_TONE) == \
        (ref.OD_SHIFT, ref.ANGLE_SHIFT, ref.SHIFT, ref.MAX_BINS, ref.MAX_TONE) == (10, 4, 16, 1024, 8192)
    # the five-header tables are as they were
    assert list(_ext.EXTENSIONS) == ['measure', 'spatial', 'outline', 'graph', 'texture'] == list(_header.EXTENSION_NAMES)
    assert len(_ext.SIGNATURES) == 15 and len(_ext.PARAMS) == 15 and len(_ext.CONSTANTS) == 22
    assert not any(k.startswith('HDY_STAIN') for k in (*_ext.CONSTANTS, *_lib.CONSTANTS))
    assert 'stain.hip' in build.SOURCES


def test_a_stain_name_belongs_to_one_header():
    from hd_yolo_amd import _ext
    both = {**_ext.EXTENSIONS, **_ext.PIXEL_EXTENSIONS}
    _ext.check_disjoint(both)                                             # the tables as they are pass
    names = [n for e in both.values() for n in (*e.functions, *e.constants)] + [*_lib.SIGNATURES, *_lib.CONSTANTS]
    assert len(names) == len(set(names))
    st = both['stain']
    with pytest.raises(_lib.HdyError) as e:
        _ext.check_disjoint(dict(both, stain=st._replace(functions=dict(st.functions, hdy_label_texture=_ext.SIGNATURES['hdy_label_texture']))))
    assert 'hdy_label_texture is declared by include/hdyolo_texture.h and by include/hdyolo_stain.h' in str(e.value)
    with pytest.raises(_lib.HdyError) as e:
        _ext.check_disjoint(dict(both, stain=st._replace(constants=dict(st.constants, HDY_ABI_VERSION=1))))
    assert 'HDY_ABI_VERSION is declared by include/hdyolo.h and by include/hdyolo_stain.h' in str(e.value)
    with pytest.raises(_lib.HdyError) as e:
        _ext.check_disjoint(dict(both, stain=st._replace(functions=dict(st.functions, hdy_slide_tissue_u8=(None, [])))))
    assert 'hdy_slide_tissue_u8 is declared by include/hdyolo.h and by include/hdyolo_stain.h' in str(e.value)


# ---- argument checks --------------------------------------------------------------------------------------------------------------------------
WS = {'moments': 1024 * 10 * 8, 'angles': 1024 * 65 * 8, 'levels': 1024 * 32 * 8}


def _count(lib, which, **kw):
    """one counting entry point on a 20 x 30 window at (2, 1) of a 40 x 50 RGB slide of 160-byte pitch: A = 64, B = 16"""
    a = dict(slide=FAKE, pitch_bytes=160, pixel_bytes=3, H=40, W=50, x0=2, y0=1, w=30, h=20, step=1, background=220, table=FAKE,
             table_elems=256 if which == 'moments' else 1536, bins=64 if which == 'angles' else 16, out=FAKE,
             out_elems={'moments': 10, 'angles': 64, 'levels': 32}[which], skipped=FAKE, skipped_elems=1, ws=FAKE, ws_bytes=WS[which])
    a.update(kw)
    head = (a['slide'], a['pitch_bytes'], a['pixel_bytes'], a['H'], a['W'], a['x0'], a['y0'], a['w'], a['h'], a['step'], a['background'],
            a['table'], a['table_elems'])
    tail = (a['ws'], a['ws_bytes'], None)
    if which == 'moments':
        rc = lib.hdy_stain_moments_u8(*head, a['out'], a['out_elems'], *tail)
    elif which == 'angles':
        rc = lib.hdy_stain_angles_u8(*head, a['bins'], a['out'], a['out_elems'], a['skipped'], a['skipped_elems'], *tail)
    else:
        rc = lib.hdy_stain_levels_u8(*head, a['bins'], a['out'], a['out_elems'], *tail)
    return rc, lib.hdy_last_error()


def _apply(lib, **kw):
    """hdy_stain_apply_u8 on the same slide and window into a disjoint 200-byte-pitch RGBA image, T = 4096"""
    a = dict(slide=FAKE, pitch_bytes=160, pixel_bytes=3, H=40, W=50, x0=2, y0=1, w=30, h=20, dst=FAKE + 0x100000, dst_pitch=200,
             dst_pixel_bytes=4, lut=FAKE, lut_elems=2304, tone=FAKE, tone_elems=4096, T=4096)
    a.update(kw)
    rc = lib.hdy_stain_apply_u8(a['slide'], a['pitch_bytes'], a['pixel_bytes'], a['H'], a['W'], a['x0'], a['y0'], a['w'], a['h'], a['dst'],
                                a['dst_pitch'], a['dst_pixel_bytes'], a['lut'], a['lut_elems'], a['tone'], a['tone_elems'], a['T'], None)
    return rc, lib.hdy_last_error()


@pytest.mark.parametrize('which', ['moments', 'angles', 'levels'])
def test_counting_passes_refuse_bad_arguments(lib, which):
    lib.hdy_dispatch_log_reset()
    bad = [({'x0': 21}, b'leaves the slide'), ({'y0': 21}, b'leaves the slide'), ({'w': 0}, b'leaves the slide'), ({'h': -1}, b'leaves the slide'),
           ({'x0': -1}, b'leaves the slide'), ({'w': 49}, b'leaves the slide'), ({'x0': 0x7fffffff, 'w': 0x7fffffff}, b'leaves the slide'),
           ({'step': 0}, b'step'), ({'step': -3}, b'step'), ({'pixel_bytes': 2}, b'pixel_bytes'), ({'pixel_bytes': 5}, b'pixel_bytes'),
           ({'pitch_bytes': 149}, b'pitch'), ({'H': 0}, b'slide of'), ({'W': (1 << 29) + 1, 'pitch_bytes': 1 << 40}, b'a side above'),
           ({'slide': None}, b'null slide'), ({'background': 257}, b'background'), ({'background': -1}, b'background'),
           ({'table': None}, b'null'), ({'table': FAKE + 2}, b'misaligned'), ({'out': None}, b'null'), ({'out': FAKE + 4}, b'misaligned'),
           ({'ws': None}, b'workspace'), ({'ws': FAKE + 4}, b'workspace'), ({'ws_bytes': WS[which] - 1}, b'ws_bytes'), ({'ws_bytes': 0}, b'ws_bytes'),
           ({'table_elems': 255}, b'_elems'), ({'table_elems': 1537}, b'_elems'), ({'table_elems': 768}, b'_elems')]
    good = {'moments': 10, 'angles': 64, 'levels': 32}[which]
    bad += [({'out_elems': n}, b'_elems') for n in (good - 1, good + 1, 0, -good)]
    if which != 'moments':
        bad += [({'bins': n}, b'outside [1, 1024]') for n in (0, -1, 1025, 1 << 20)]
    if which == 'angles':
        bad += [({'skipped': None}, b'null'), ({'skipped_elems': 0}, b'skipped_elems'), ({'skipped_elems': 2}, b'skipped_elems')]
    for kw, word in bad:
        rc, msg = _count(lib, which, **kw)
        assert rc == _lib.EINVAL and word in msg and f'stain_{which}'.encode() in msg, (kw, msg)
    assert _lib.dispatch_log() == []


def test_apply_refuses_bad_arguments(lib):
    lib.hdy_dispatch_log_reset()
    bad = [({'x0': 21}, b'leaves the slide'), ({'h': 40}, b'leaves the slide'), ({'w': 0}, b'leaves the slide'), ({'pixel_bytes': 1}, b'pixel_bytes'),
           ({'dst_pixel_bytes': 2}, b'dst_pixel_bytes'), ({'dst_pixel_bytes': 5}, b'dst_pixel_bytes'), ({'dst': None}, b'null dst'),
           ({'dst_pitch': 199}, b'dst_pitch'), ({'T': 0}, b'T=0'), ({'T': 8193, 'tone_elems': 8193}, b'T=8193'), ({'tone_elems': 4095}, b'tone_elems'),
           ({'lut_elems': 1536}, b'lut_elems'), ({'lut': None}, b'null'), ({'lut': FAKE + 1}, b'misaligned'), ({'tone': None}, b'null tone'),
           # overlap: the slide itself but another pitch or pixel size, a shifted start, the end of dst inside the slide
           ({'dst': FAKE, 'dst_pitch': 200, 'dst_pixel_bytes': 3}, b'overlaps'), ({'dst': FAKE, 'dst_pitch': 200}, b'overlaps'),
           ({'dst': FAKE + 160, 'dst_pitch': 160, 'dst_pixel_bytes': 3}, b'overlaps'), ({'dst': FAKE - 200 * 39 - 1}, b'overlaps'),
           ({'dst': FAKE + 39 * 160 + 149}, b'overlaps')]
    for kw, word in bad:
        rc, msg = _apply(lib, **kw)
        assert rc == _lib.EINVAL and word in msg and b'stain_apply' in msg, (kw, msg)
    assert _lib.dispatch_log() == []


# ---- bounds, over all 256 values ---------------------------------------------------------------------------------------------------------------
def test_angle_arithmetic_stays_inside_32_bits_for_every_unit_vector():
    """|entry| <= 2^10 e q(0) for a component e of a unit vector, so |sum of three| <= 2^10 q(0) (|e_R| + |e_G| + |e_B|) <= 2^10 * 2466 * sqrt(3):
    from the table's maximum, not from a sample of vectors."""
    q = ref.od_table()
    assert q[0] == 2466 and q[255] == 0 and (np.diff(q) <= 0).all() and np.array_equal(q, hstain.od_table().numpy())
    top = (1 << 10) * int(q.max())
    assert hstain.plane_lut((1, 0, 0), (0, -1, 0)).abs().max().item() == top                          # the bound of an entry is reached
    p_max = (math.ceil(math.sqrt(3) * top) + 2) >> ref.ANGLE_SHIFT                                    # + 2: three roundings of half a unit
    assert p_max < 1 << 20
    s_max = 2 * p_max
    assert ref.MAX_BINS * (s_max + p_max) < 1 << 32 and ref.MAX_BINS * 2 * s_max < 1 << 32


def test_the_bin_never_reaches_A():
    # p_1 < s whenever p_0 > 0, so s + p_1 < 2 s: at the extremes of p_1 against p_0 = 1, at p_1 = 0, and at the largest magnitudes
    big = (1 << 20) - 1
    p0 = np.array([1, 1, 1, big, big, 1, 7, big], np.int64)
    p1 = np.array([big, -big, 0, big, -big, 1, -3, 0], np.int64)
    for A in (1, 2, 3, 64, 1000, 1024):
        b = ref.angle_bins(p0, p1, A)
        assert b.min() >= 0 and b.max() < A
        assert b[1] == 0 and b[0] == A - 1 and b[2] == A // 2
    # monotone in the angle
    rng = np.random.default_rng(0)
    p0, p1 = rng.integers(1, big, 4000), rng.integers(-big, big, 4000)
    order = np.argsort(np.arctan2(p1, p0), kind='stable')
    assert (np.diff(ref.angle_bins(p0[order], p1[order], 1024)) >= 0).all()


def test_three_level_or_apply_entries_cannot_wrap():
    for (h, e), _ in PAIRS:
        lut = hstain.level_lut(_matrix(h, e), 1024, 4.0)
        assert lut.dtype == torch.int32 and tuple(lut.shape) == (2, 3, 256) and 3 * int(lut.abs().max()) < 1 << 31
        for s, name in enumerate(('hematoxylin', 'eosin')):                # B = 16, c_top = od_max: texture.stain_lut's table
            assert torch.equal(hstain.level_lut(_matrix(h, e), 16, 2.0)[s], htexture.stain_lut(name, 16, od_max=2.0, matrix=_matrix(h, e)))
    est = hstain.StainEstimate(torch.from_numpy(_matrix(*PAIRS[1][0])), torch.tensor([0.5, 0.3]), 100, 0, 0)
    lut, tone = hstain.normalizer(est)
    assert tuple(lut.shape) == (3, 3, 256) and tone.numel() == 8192
    assert int(lut.to(torch.int64).abs().amax(2).sum(1).max()) < 1 << 31
    with pytest.raises(ValueError):                                       # a ratio of 30: three entries could pass 2^31
        hstain.normalizer(est._replace(max_conc=torch.tensor([0.03, 0.3])))
    with pytest.raises(ValueError):                                       # nearly parallel vectors: an entry reaches 2^28
        hstain.level_lut(_matrix(M0[0], _rot(M0[0], (0, 0, 1), 1e-4)), 1024, 4.0)
    for bad in (dict(B=0), dict(B=1025)):
        with pytest.raises(ValueError):
            hstain.level_lut(M0, c_top=4.0, **bad)


# ---- the restatement and the estimator on synthetic slides -----------------------------------------------------------------------------------
ANGLE_BIN_DEG = math.degrees(2 / 1024)
LEVEL_BIN = 4.0 / 1024


@pytest.mark.parametrize('k', [0, 1, 2])
def test_estimate_on_synthetic_slides_against_the_ideal(k):
    """The integer method may be worse than the float64 ideal on the same image by one angle bin (2 / A rad = 0.112 degrees at A = 1024) and one
    level bin (c_top / B = 0.0039).  Measured here (384 x 384, seeds 0 .. 2; errors against the vectors and concentrations the slide was drawn
    with): ideal 0.13 to 0.16 degrees on haematoxylin and 0.35 to 0.43 on eosin, 0.0003 to 0.0047 on the concentrations; the integer method
    0.15 to 0.20 and 0.30 to 0.44 degrees, 0.0004 to 0.0059.  Both printed below."""
    (h, e), conc = PAIRS[k]
    img = synth.synth_stained_slide(384, np.stack([h, e]), conc, seed=k)
    assert img.dtype == np.uint8 and img.shape == (384, 384, 3) and (img[-1] == 255).all()
    mi, ci = ref.ideal_estimate(img)
    est = hstain.estimate_from_counts(ref.RefCounts(img))
    assert est.flags == 0 and est.n_tissue == int((img.min(2) < 220).sum()) and est.n_skipped == 0
    m = est.matrix.numpy()
    np.testing.assert_allclose(np.linalg.norm(m, axis=1), 1.0, atol=1e-12)
    assert abs(m[2] @ m[0]) < 1e-12 and abs(m[2] @ m[1]) < 1e-12
    for s, true in enumerate((h, e)):
        ideal_err, got_err = ref.angle_deg(mi[s], true), ref.angle_deg(m[s], true)
        print(f'pair {k} stain {s}: ideal {ideal_err:.4f} deg, integer {got_err:.4f} deg; concentration ideal {ci[s] - conc[s]:+.5f}, '
              f'integer {float(est.max_conc[s]) - conc[s]:+.5f}')
        assert ideal_err < 1.0                                            # the synthetic slide does determine its vectors
        assert got_err <= ideal_err + ANGLE_BIN_DEG
        assert abs(float(est.max_conc[s]) - conc[s]) <= abs(ci[s] - conc[s]) + LEVEL_BIN


def test_counts_of_windows_and_steps_follow_the_definition():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (23, 31, 4)).astype(np.uint8)
    od = ref.od_table()
    s = ref.moments(img, od, (3, 2, 20, 17), 3, 200)
    px = np.array([img[y, x, :3] for y in range(2, 19, 3) for x in range(3, 23, 3)]).astype(np.int64)
    px = px[px.min(1) < 200]
    assert s[0] == len(px) and s[1] == od[px[:, 0]].sum() and s[8] == (od[px[:, 1]] * od[px[:, 2]]).sum()
    assert ref.moments(img, od, (3, 2, 20, 17), 100, 256)[0] == 1          # a step beyond the window: its first pixel
    lut = hstain.plane_lut(M0[0], M0[1]).numpy()
    hist, skipped = ref.angles(img, lut, 64, (3, 2, 20, 17), 3, 200)
    assert hist.sum() + skipped[0] == len(px)
    lv = ref.levels(img, hstain.level_lut(M0, 16, 2.0).numpy(), 16, (3, 2, 20, 17), 3, 200)
    assert lv.shape == (2, 16) and (lv.sum(1) == len(px)).all()
    assert ref.wrap32(np.array([(1 << 31), -(1 << 31) - 1, 5])).tolist() == [-(1 << 31), (1 << 31) - 1, 5]


# ---- the estimator's rules -------------------------------------------------------------------------------------------------------------------
def test_percentile_rule_on_hand_made_histograms():
    pb = lambda h, k: hstain.percentile_bin(torch.tensor(h), k)          # noqa: E731
    assert [hstain.rank(a, n) for a, n in ((0.01, 100), (0.01, 101), (0.99, 100), (0.07, 100), (0.01, 2), (0.99, 2), (0.5, 3), (0.01, 1))] == \
        [1, 2, 99, 7, 1, 2, 2, 1] == [ref.rank(a, n) for a, n in ((0.01, 100), (0.01, 101), (0.99, 100), (0.07, 100), (0.01, 2), (0.99, 2), (0.5, 3), (0.01, 1))]
    assert pb([0, 0, 5, 0], 1) == 2 and pb([0, 0, 5, 0], 5) == 2           # all mass in one bin
    assert pb([2, 0, 2, 0], 2) == 0 and pb([2, 0, 2, 0], 3) == 2           # ties: the lowest bin that reaches the count
    assert pb([1, 0, 0, 1], hstain.rank(0.01, 2)) == 0 and pb([1, 0, 0, 1], hstain.rank(0.99, 2)) == 3      # n = 2
    assert pb([1, 1], 5) == 1                                              # a count never reached: the last bin
    for A in (1, 7, 1024):                                                 # the bin centre goes back to the angle whose bin it is
        for b in range(0, A, max(1, A // 13)):
            phi = hstain.bin_angle(b, A)
            p0, p1 = int(round(1e5 * math.cos(phi))), int(round(1e5 * math.sin(phi)))
            assert -math.pi / 2 < phi < math.pi / 2 and ref.angle_bins(np.array([p0]), np.array([p1]), A)[0] == b


class _Counts:
    """hand-made counts behind the three calls"""

    def __init__(self, sums, hist=None, skipped=0, levels=None):
        self.sums, self.hist, self.skipped, self.lv, self.calls = sums, hist, skipped, levels, []

    def moments(self, od):
        self.calls.append('moments')
        return torch.tensor(self.sums, dtype=torch.int64)

    def angles(self, lut, A):
        self.calls.append('angles')
        return torch.tensor(self.hist, dtype=torch.int64), torch.tensor([self.skipped], dtype=torch.int64)

    def levels(self, lut, B):
        self.calls.append('levels')
        return torch.tensor(self.lv, dtype=torch.int64)


def test_flags_and_identity_on_a_flag():
    target = hstain.StainTarget()
    assert torch.equal(target.matrix, htexture.stain_matrix()) and target.max_conc.tolist() == [0.8558, 0.4477]
    np.testing.assert_allclose(target.max_conc.numpy() * math.log(10), [1.9705, 1.0308], atol=2e-4)      # Macenko's reference, natural logarithm
    # 1: fewer than two tissue pixels (an all-background slide, a single pixel)
    white = np.full((8, 8, 3), 255, np.uint8)
    one = white.copy()
    one[3, 3] = (90, 60, 140)
    for img, n in ((white, 0), (one, 1)):
        est = hstain.estimate_from_counts(ref.RefCounts(img))
        assert (est.flags, est.n_tissue, est.n_skipped) == (1, n, 0)
    # 2: a covariance of rank below 2: one colour, and colours on one line of optical density
    flat = np.full((8, 8, 3), 100, np.uint8)
    c = _Counts([0] * 10)
    line = np.stack([np.full((8, 8), v, np.uint8) for v in (40, 40, 40)], 2)
    line[::2] = 90
    for img in (flat, line):
        est = hstain.estimate_from_counts(ref.RefCounts(img))
        assert (est.flags, est.n_tissue) == (2, 64)
    # 3: the level table is refused: both percentile bins equal, the two vectors are the same
    sums = ref.moments(synth.synth_stained_slide(64, M0[:2], (0.8, 0.4)), ref.od_table()).tolist()
    hist = [0] * 16
    hist[9] = 50
    c = _Counts(sums, hist)
    est = hstain.estimate_from_counts(c, bins=16)
    assert est.flags == 3 and c.calls == ['moments', 'angles'] and est.n_tissue == sums[0]
    # the flags are exclusive and in order; every flagged estimate is the target, and normalising with it is the identity up to quantisation
    assert torch.equal(est.matrix, target.matrix) and torch.equal(est.max_conc, target.max_conc)
    np.testing.assert_allclose(hstain.transfer_matrix(est).numpy() @ M0[:2].T, M0[:2].T, atol=1e-12)      # both stain vectors are fixed points
    with pytest.raises(ValueError):
        hstain.estimate_from_counts(c, alpha=0.5)
    with pytest.raises(ValueError):
        hstain.estimate_from_counts(c, bins=1025)


def test_tone_table():
    for T in (8192, 4096, 100, 1):
        t = hstain.tone_table(T).numpy().astype(int)
        assert t.shape == (T,) and (np.diff(t) <= 0).all() and t[0] == {8192: 255, 4096: 255, 100: 248, 1: 15}[T] and (t[-1] == 0 or T == 1)
    t = hstain.tone_table(8192).numpy().astype(int)
    assert set(range(256)) == set(t.tolist()) and np.diff(t).min() == -1          # every byte is reached, none is jumped over
    assert 256 * math.log(10) * ref.OD_TOP / 8192 < 0.18                          # the table's step in bytes
    for bad in (0, 8193):
        with pytest.raises(ValueError):
            hstain.tone_table(bad)


@pytest.fixture(scope='module')
def slide_and_estimate():
    (h, e), conc = PAIRS[1]
    img = synth.synth_stained_slide(192, np.stack([h, e]), conc, seed=7)
    return img, hstain.estimate_from_counts(ref.RefCounts(img))


def test_recolouring_to_the_own_stains_changes_no_byte_by_more_than_one(slide_and_estimate):
    img, est = slide_and_estimate
    # estimate == target, and a matrix without a dropped residual: the identity map, so every byte moves by the quantisation alone
    lut, tone = hstain.apply_lut(np.eye(3), 8192), hstain.tone_table(8192)
    out = ref.apply(img, lut.numpy(), tone.numpy())
    assert out.dtype == np.uint8 and np.abs(out.astype(int) - img.astype(int)).max() <= 1
    # with the slide's own estimate as the target the two-stain map is the identity on the stain plane: the synthetic slide lies in it up
    # to its rounding and the estimate's error, which the ideal recolouring shares
    lut, tone = hstain.normalizer(est, hstain.StainTarget(est.matrix, est.max_conc))
    out = ref.apply(img, lut.numpy(), tone.numpy())
    ideal = ref.ideal_recolour(img, hstain.transfer_matrix(est, hstain.StainTarget(est.matrix, est.max_conc)).numpy())
    assert np.abs(out.astype(int) - np.rint(ideal).astype(int)).max() <= 1
    assert np.abs(out.astype(int) - img.astype(int)).max() <= 1            # estimate == target: no byte changes by more than 1


def test_recolouring_is_within_one_of_the_rounded_ideal(slide_and_estimate):
    """stain_ref's docstring derives the bound; here over every pixel of a slide of turned stains recoloured to the default target, and over
    an image of random colours (far from the stain plane, negative optical densities and indices beyond both ends included)"""
    img, est = slide_and_estimate
    rnd = np.random.default_rng(11).integers(0, 256, (64, 64, 3)).astype(np.uint8)
    lut, tone = hstain.normalizer(est)
    N = hstain.transfer_matrix(est).numpy()
    for image in (img, rnd):
        out = ref.apply(image, lut.numpy(), tone.numpy())
        worst = np.abs(out.astype(int) - np.rint(ref.ideal_recolour(image, N)).astype(int)).max()
        print('largest difference from the rounded ideal:', worst)
        assert worst <= 1
    assert (ref.apply(rnd, lut.numpy(), tone.numpy()) == 255).any() and (ref.apply(rnd, lut.numpy(), tone.numpy()) == 0).any()
    assert not np.array_equal(ref.apply(img, lut.numpy(), tone.numpy()), img)
    # alpha: copied where the source has one, 255 where only the destination has
    rgba = np.concatenate([img, np.full(img.shape[:2] + (1,), 9, np.uint8)], 2)
    assert (ref.apply(rgba, lut.numpy(), tone.numpy())[..., 3] == 9).all() and (ref.apply(img, lut.numpy(), tone.numpy(), out_channels=4)[..., 3] == 255).all()


# ---- the matrix hook of the texture table ----------------------------------------------------------------------------------------------------
def test_texture_table_passes_the_matrix_to_stain_lut(monkeypatch):
    from hd_yolo_amd import ops
    rng = np.random.default_rng(4)
    lm = rng.integers(-1, 5, (24, 30)).astype(np.int32)
    rgb = synth.synth_stained_slide(32, np.stack(PAIRS[2][0]), PAIRS[2][1], tissue=1.0, seed=2)[:24, :30]
    ext = np.tile(np.array([[0, 0, 29, 23]], np.int32), (5, 1))

    def cpu_label_texture(label_map, R, extent, image, lut, levels, offsets, window, rows):
        out = texture_ref.texture_vec(label_map.numpy(), image.numpy(), extent.numpy(), lut.numpy(), levels, offsets, row0=rows[0], rows=rows[1])
        return tuple(torch.from_numpy(v) for v in out)

    monkeypatch.setattr(ops, 'label_texture', cpu_label_texture)
    M = torch.from_numpy(_matrix(*PAIRS[2][0]))
    args = (torch.from_numpy(lm), 5, torch.from_numpy(ext), torch.from_numpy(rgb))
    got = htexture.texture_table(*args, stain='eosin', matrix=M)
    plain = htexture.texture_table(*args, stain='eosin')
    real = htexture.stain_lut
    monkeypatch.setattr(htexture, 'stain_lut', lambda stain, levels, od_max=None, matrix=None, device=None: real(stain, levels, od_max, M, device))
    want = htexture.texture_table(*args, stain='eosin')
    assert set(got) == set(want) and all(torch.equal(torch.nan_to_num(got[k], nan=-7.0), torch.nan_to_num(want[k], nan=-7.0)) for k in want)
    assert not torch.equal(got['tex_level_mean'], plain['tex_level_mean'])      # the matrix does change the columns
