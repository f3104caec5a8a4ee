"""CPU only.  Pins tests/pool_ref.py (the restatement the direct tests of csrc/pool.hip compare with) to ATen on the CPU: values and indices of
three chained F.max_pool2d(5, 1, 2, return_indices=True) in fp32 and bf16 on every case of tests/pool_cases.py, special values included; the
position bytes decode to those indices; the 'first' NaN policy differs from ATen's only inside NaN windows and names the first NaN there; the
float64 backward equals float64 autograd; upsample, stem_prep and nchw_to_nhwc equal F.interpolate and its autograd, F.pad plus cast, permute
plus cast.  It proves that the selection rules restated in pool_cases are those of the launchers' text, that every case reaches the variant it
is listed for and every boundary case sits on its boundary, and that the bounds reject a misrouted gradient and a bf16 ulp."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pool_cases as pc
import pool_ref as ref

SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'hd_yolo_amd', 'csrc', 'pool.hip')).read()
TORCH = {'f32': torch.float32, 'bf16': torch.bfloat16}
CASES = pc.sppf_cases()


def nchw(a, dt=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).permute(0, 3, 1, 2).contiguous()
    return t.to(TORCH[dt]) if dt else t


def nhwc(t):
    return t.detach().float().permute(0, 2, 3, 1).contiguous().numpy() if t.dtype != torch.int64 else t.permute(0, 2, 3, 1).contiguous().numpy()


# ------------------------------------------------------------------------------------------ the launchers' text
def test_selection_rules_are_those_of_the_launchers_text():
    assert re.search(r'constexpr int CG = (\d+);', SRC).group(1) == str(pc.CG) and re.search(r'constexpr int PB = (\d+);', SRC).group(1) == str(pc.PB)
    assert SRC.count('150 * 1024') >= 10 and pc.LDS == 150 * 1024
    assert 'const size_t pix = (size_t)(H + 2 * PB) * (W + 2 * PB);' in SRC
    for cg in (32, 16):                                            # keys first, then the float-compare kernels, 32 before 16, the same fit test
        fit = f'C % {cg} == 0 && pix * {cg} * (2 * sizeof(bf16_t) + ix) <= 150 * 1024)'
        assert f'if (keys && {fit}' in SRC and f'if ({fit}' in SRC
    order = [SRC.index(s) for s in ('sppf_fwd_keys_launch<32, 1024>(x', 'sppf_fwd_keys_launch<16, 1024>(x', 'sppf_fwd_launch<bf16_t, bf16_t, 32, 1024>(x',
                                    'sppf_fwd_launch<bf16_t, bf16_t, 16, 1024>(x', 'sppf_fwd_launch<bf16_t, float, CG, 256>(x', 'sppf_fwd_launch<float, float, CG, 256>(x')]
    assert order == sorted(order)
    assert 'const bool keys = !hdy_opt(HDY_OPT_SPPF_NO_KEYS)' in SRC
    assert SRC.count('const size_t smem = pix * CG * (2 * sizeof(float) + ix);') == 2
    assert 'if (dtype == HDY_BF16 && C % 16 == 0 && pix * 16 * (2 * sizeof(float) + 2) <= 150 * 1024)' in SRC
    assert 'const int two_ix = plane * (2 * sizeof(float) + 2) <= 150 * 1024;' in SRC and 'const size_t plane = pix * CG;' in SRC
    assert 'const size_t smem = plane * (2 * sizeof(float) + (two_ix ? 2 : 1));' in SRC
    assert 'if (g > 4096) g = 4096;' in SRC and pc.GRID_CAP == 4096 * 256
    for name in pc.FWD_NAMES + pc.BWD_NAMES:
        assert f'"{name}"' in SRC, f'{name} is not a name the launchers log'
    assert pc.LIMIT == {'fwd32_pos': 960, 'fwd16_pos': 1920, 'fwd8_pos': 2133, 'fwd32': 1200, 'fwd16': 2400, 'fwd8': 2400, 'bwd16': 960,
                        'bwd8_two': 1920, 'bwd8_one': 2133}


def _claims(desc, H, W):
    p = pc.pix(H, W)
    for how, key in re.findall(r'\b(one past|past|below|at) ((?:fwd|bwd)\w+)', desc):
        lim = pc.LIMIT[key]
        assert {'at': p == lim, 'one past': p == lim + 1, 'past': p > lim, 'below': p <= lim}[how], (desc, p, lim)
    if 'at its limit' in desc:
        key = re.search(r'(bwd\w+) at its limit', desc).group(1)
        assert p == pc.LIMIT[key], (desc, p)


@pytest.mark.parametrize('dt', pc.DTYPES)
def test_every_case_reaches_the_variant_it_is_listed_for(dt):
    for positions, table in ((True, pc.TRAIN[dt]), (False, pc.INFER[dt])):
        for (N, H, W, C), desc in table:
            assert 1 <= N <= 3
            want = desc.split()[0].rstrip(':;')
            if want.startswith('bwd'):
                want = 'c8'
            assert pc.fwd_variant(dt, H, W, C, positions) == f'sppf_fwd_{want}' + ('_pos' if positions else ''), desc
            for key in re.findall(r'\b(bwd16|bwd8_two|bwd8_one)\b', desc):
                if f'past {key}' not in desc and f'below {key}' not in desc:
                    assert pc.bwd_variant(dt, H, W, C) == 'sppf_bwd_' + key.replace('bwd', 'c'), desc
            _claims(desc, H, W)
            if want.startswith('keys'):                          # the same shape reaches the float-compare kernel of the same width
                assert pc.fwd_variant(dt, H, W, C, positions, no_keys=True) == f'sppf_fwd_float{want[4:]}' + ('_pos' if positions else '')


def test_every_variant_and_form_has_a_case_and_the_refused_planes_do_not_fit():
    seen_f, seen_b = set(), set()
    for _, dt, (N, H, W, C), _, _, positions in CASES:
        for nk in (False, True):
            seen_f.add(pc.fwd_variant(dt, H, W, C, False, nk))
            if positions:
                seen_f.add(pc.fwd_variant(dt, H, W, C, True, nk))
                seen_b.add(pc.bwd_variant(dt, H, W, C))
    assert seen_f == set(pc.FWD_NAMES) and seen_b == set(pc.BWD_NAMES)
    for dt, (N, H, W, C), positions in pc.REFUSED_FWD:
        assert pc.fwd_variant(dt, H, W, C, positions) is None and pc.fwd_variant(dt, H, W, C, positions, True) is None
    for dt, (N, H, W, C) in pc.REFUSED_BWD:
        assert pc.bwd_variant(dt, H, W, C) is None
    assert pc.pix(18, 93) == pc.LIMIT['fwd8_pos'] + 1 and pc.pix(45, 45) == pc.LIMIT['fwd8'] + 1 and pc.pix(43, 42) == 2162
    for dt, shape in (pc.UP_BIG_FWD, pc.UP_BIG_BWD):
        fwd = (dt, shape) == pc.UP_BIG_FWD
        assert pc.GRID_CAP < pc.up_vectors(dt, shape, fwd) < pc.GRID_CAP * 1.02
    B, H, W, pad = pc.STEM_BIG
    assert pc.GRID_CAP < B * (H + 2 * pad) * (W + 2 * pad) < pc.GRID_CAP * 1.01
    for dt in pc.DTYPES:
        assert all(pc.up_vectors(dt, s, True) <= pc.GRID_CAP for _, d, s, _ in pc.upsample_cases() if d == dt)
        assert {s[3] // pc.VE[dt] for _, d, s, _ in pc.upsample_cases() if d == dt} >= {1}
    assert sorted(h * w for h, w in pc.LAYOUT_HW) == [1, 31, 32, 33, 99]


# ------------------------------------------------------------------------------------------ SPPF against ATen
def aten_chain(x, dt):
    t = nchw(x, dt)
    ys, idxs = [], []
    for _ in range(3):
        t, i = F.max_pool2d(t, 5, 1, 2, return_indices=True)
        ys.append(nhwc(t))
        idxs.append(nhwc(i))
    return ys, idxs


@pytest.mark.parametrize('case', CASES, ids=[c[0] for c in CASES])
def test_forward_values_indices_and_position_bytes_are_atens(case):
    _, dt, shape, fam, _, _ = case
    x = pc.family(fam, dt, shape)
    if fam != 'random':
        assert {'nan': np.isnan(x).any(), 'pinf': (x == np.inf).any(), 'ninf': (x == -np.inf).any(), 'zeros': (np.signbit(x) & (x == 0)).any(),
                'ties': True, 'const': True}[next(k for k in ('nan', 'pinf', 'ninf', 'zeros', 'ties', 'const') if fam.startswith(k))]
    ys, idxs, poss = ref.sppf_fwd(x, 'last')
    for dtt in pc.DTYPES if dt == 'bf16' else ('f32',):          # bf16 values are fp32 values too: both of ATen's kernels
        ay, ai = aten_chain(x, dtt)
        for lv in range(3):
            assert ref.same_bits(ys[lv], ay[lv], nan_payload=False).all(), f'level {lv + 1} values ({dtt})'
            assert np.array_equal(idxs[lv], ai[lv]), f'level {lv + 1} indices ({dtt})'
    for lv in range(3):
        assert np.array_equal(ref.decode(poss[lv]), idxs[lv]), f'level {lv + 1}: the position bytes decode to other indices'
    # the keys' policy: the same values, other positions only where the window holds a NaN, and there the first NaN in row-major order
    fy, fi, fp = ref.sppf_fwd(x, 'first')
    src = x
    for lv in range(3):
        nanw = np.isnan(ys[lv])
        assert ref.same_bits(fy[lv], ys[lv], nan_payload=False).all()
        assert np.array_equal(fi[lv][~nanw], idxs[lv][~nanw]) and np.array_equal(fp[lv][~nanw], poss[lv][~nanw])
        assert np.array_equal(ref.decode(fp[lv]), fi[lv])
        if nanw.any():
            N, H, W, C = shape
            flat = np.isnan(src).reshape(N, H * W, C)
            for n, h, w, c in np.argwhere(nanw)[:200]:
                in_win = [r * W + cc for r in range(max(h - 2, 0), min(h + 3, H)) for cc in range(max(w - 2, 0), min(w + 3, W)) if flat[n, r * W + cc, c]]
                assert fi[lv][n, h, w, c] == in_win[0] and idxs[lv][n, h, w, c] == in_win[-1]
        src = ys[lv]
    if fam == 'zeros':
        assert any((np.signbit(y) & (y == 0)).any() for y in ys) and (np.signbit(ys[2][..., 1])).all(), 'no -0-only window'
    if fam == 'nan_window':
        assert (np.isnan(x[0, 3:10, 2:10, 0]).sum() >= 5)


@pytest.mark.parametrize('case', [c for c in CASES if c[5]], ids=[c[0] for c in CASES if c[5]])
def test_backward_equals_float64_autograd(case):
    _, dt, shape, fam, _, _ = case
    x = pc.family(fam, dt, shape)
    gs = pc.grads(dt, shape)
    _, idxs, _ = ref.sppf_fwd(x, 'last')
    dx, A = ref.sppf_bwd(gs, idxs)
    t = nchw(x).double().requires_grad_(True)
    y1 = F.max_pool2d(t, 5, 1, 2)
    y2 = F.max_pool2d(y1, 5, 1, 2)
    y3 = F.max_pool2d(y2, 5, 1, 2)
    torch.autograd.backward([y1, y2, y3], [nchw(g).double() for g in gs[1:]])          # a pool's backward only scatters: NaN inputs make no NaN gradients
    want = (t.grad + nchw(gs[0]).double()).permute(0, 2, 3, 1).numpy()
    assert np.abs(dx - want).max() <= 1e-12 * max(np.abs(want).max(), 1.0)
    assert (A >= np.abs(dx) - 1e-12).all() and abs(dx.sum() - sum(g.astype(np.float64).sum() for g in gs)) <= 1e-9
    # non-vacuous: one gradient routed one pixel off, or a bf16 ulp, lies outside the bound
    bound = ref.sppf_bwd_bound(A, dt == 'bf16', dx)
    N, H, W, C = shape
    n, h, w, c = np.unravel_index(int(np.argmax(np.abs(gs[1]))), dx.shape)             # the largest level-1 gradient, sent to the pixel after its target
    off = dx.copy().reshape(N, H * W, C)
    off[n, idxs[0][n, h, w, c], c] -= float(gs[1][n, h, w, c])
    off[n, (idxs[0][n, h, w, c] + 1) % (H * W), c] += float(gs[1][n, h, w, c])
    assert H * W == 1 or ref.ratios(off.reshape(shape), dx, bound).max() > 1.0
    k = np.unravel_index(int(np.argmax(np.abs(dx))), dx.shape)
    ulp = dx.copy()
    ulp[k] *= 1 + 2.0 ** -7
    assert ref.ratios(ulp, dx, bound).max() > 1.0
    r32 = ref.ratios(ref.q(ref.sppf_bwd(gs, idxs, np.float32)[0], dt), dx, bound)
    assert r32.max() <= 1.0
    print(f'POOLFIG-CPU sppf bwd {dt} | {case[0]} | {r32.max():.3f}')


def test_integer_gradients_are_exact_in_fp32():
    shape = (2, 12, 13, 8)
    x = pc.family('ties', 'f32', shape)
    gs = pc.grads('f32', shape, integer=True)
    _, idxs, _ = ref.sppf_fwd(x)
    d64, A = ref.sppf_bwd(gs, idxs)
    assert A.max() < 2 ** 24 and np.array_equal(ref.sppf_bwd(gs, idxs, np.float32)[0].astype(np.float64), d64)


# ------------------------------------------------------------------------------------------ upsample, stem_prep, nchw_to_nhwc
@pytest.mark.parametrize('case', pc.upsample_cases(), ids=[c[0] for c in pc.upsample_cases()])
def test_upsample_restatement_is_interpolate_and_its_autograd(case):
    _, dt, shape, _ = case
    N, H, W, C = shape
    x = pc.up_input(dt, shape, 1, special=True)
    want = F.interpolate(nchw(x), scale_factor=2.0, mode='nearest')
    assert np.array_equal(ref.bits(ref.upsample_fwd(x)), ref.bits(nhwc(want)))
    dy = pc.up_input(dt, (N, 2 * H, 2 * W, C), 2)
    old = pc.up_input(dt, shape, 3)
    t = nchw(x).double().nan_to_num(0.0, 0.0, 0.0).requires_grad_(True)
    F.interpolate(t, scale_factor=2.0, mode='nearest').backward(nchw(dy).double())
    for o in (None, old):
        dx, A = ref.upsample_bwd(dy, o)
        w = t.grad.permute(0, 2, 3, 1).numpy() + (0 if o is None else o.astype(np.float64))
        assert np.abs(dx - w).max() <= 1e-12 * max(np.abs(w).max(), 1.0) and (A >= np.abs(dx) - 1e-12).all()
        bound = ref.upsample_bwd_bound(A, dt == 'bf16', dx)
        k = np.unravel_index(int(np.argmax(np.abs(dx))), dx.shape)
        bad = dx.copy()
        bad[k] *= 1 + 2.0 ** -7
        assert ref.ratios(bad, dx, bound).max() > 1.0
        r32 = ref.ratios(ref.q(ref.upsample_bwd(dy, o, np.float32)[0], dt), dx, bound)
        assert r32.max() <= 1.0
        print(f'POOLFIG-CPU upsample bwd {dt} | {case[0]} {"acc" if o is not None else "store"} | {r32.max():.3f}')
    sp = pc.up_input(dt, (N, 2 * H, 2 * W, C), 4, special=True)
    dx, _ = ref.upsample_bwd(sp, None)
    s32 = nchw(sp).view(N, C, H, 2, W, 2)
    w32 = (s32[:, :, :, 0, :, 0] + s32[:, :, :, 0, :, 1] + s32[:, :, :, 1, :, 0] + s32[:, :, :, 1, :, 1]).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(np.isnan(dx), np.isnan(w32)) and np.array_equal(np.isinf(dx), np.isinf(w32))


@pytest.mark.parametrize('dt', pc.DTYPES)
def test_stem_prep_and_nchw_to_nhwc_restatements(dt):
    for B, H, W, pad in pc.STEM:
        img = pc.image((B, 3, H, W), H)
        want = F.pad(torch.from_numpy(img).permute(0, 2, 3, 1), (0, 1, pad, pad, pad, pad)).to(TORCH[dt]).float().numpy()
        got = ref.stem_prep(img, pad, dt)
        assert got.shape == (B, H + 2 * pad, W + 2 * pad, 4) and ref.same_bits(got, want, nan_payload=False).all()
    for C in pc.LAYOUT_C:
        for k, (H, W) in enumerate(pc.LAYOUT_HW):
            src = pc.image((1 + k % 3, C, H, W), C + k)
            want = torch.from_numpy(src).permute(0, 2, 3, 1).to(TORCH[dt]).float().numpy()
            assert ref.same_bits(ref.nchw_to_nhwc(src, dt), want, nan_payload=False).all()
