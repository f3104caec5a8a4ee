"""Host side of the device AP matching, no GPU: the numpy restatement of its five steps (tests/score_ref.py) gives the stats of
APMeter.ap_per_class on the reference-made inputs of tests/golden/f3.npz and on random images with ignored labels and empty images; the
cell-binned form equals the dense form; the chunk-box visit count; and the ABI surface of hdy_ap_match answers invalid calls by status."""
import ctypes
import os

import numpy as np
import pytest
import torch

import score_ref as ref
from hd_yolo_amd import _lib, build
from metayolo.models.metrics import APMeter

G = np.load(os.path.join(os.path.dirname(__file__), 'golden', 'f3.npz'), allow_pickle=False)
STAT_KEYS = ('ap', 'p', 'r', 'f1', 'py')


def assert_same_stats(a, b):
    assert [int(v) for v in a['labels']] == [int(v) for v in b['labels']]
    assert [int(v) for v in a['counts']] == [int(v) for v in b['counts']]
    for k in STAT_KEYS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


def f3_images():
    i, out = 0, []
    while f'ap_in_{i}_o_boxes' in G:
        out.append(({k: torch.from_numpy(G[f'ap_in_{i}_o_{k}']) for k in ('boxes', 'scores', 'labels')},
                    {k: torch.from_numpy(G[f'ap_in_{i}_t_{k}']) for k in ('boxes', 'labels')}))
        i += 1
    assert i == 6
    return out


@pytest.mark.parametrize('ignore', [(-100, -1), ()])
def test_restatement_equals_apmeter_on_the_reference_inputs(ignore):
    host, mine = APMeter(), ref.RefMeter(ignore=ignore)
    for o, t in f3_images():
        s = o['scores'].numpy()
        assert len(np.unique(s)) == len(s), 'the comparison needs distinct scores per image (the tie rule is where the two may differ)'
        host.add(o, t)
        mine.add(o, t)
    want = host.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=list(ignore))
    assert_same_stats(mine.ap_per_class(), want)
    tag = 'default' if ignore else 'noignore'
    np.testing.assert_allclose(mine.ap_per_class()['ap'], G[f'ap_{tag}_ap'], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize('ignore', [(-100, -1), ()])
def test_restatement_equals_apmeter_on_random_images(ignore):
    rng = np.random.default_rng(11)
    host, mine = APMeter(), ref.RefMeter(ignore=ignore)
    n_images = n_pairs = n_touched = 0
    shapes = [(0, 0), (0, 7), (9, 0)] + [(int(rng.integers(1, 200)), int(rng.integers(1, 250))) for _ in range(42)]
    for n, m in shapes:
        pb, ps, pl, tb, tl = ref.random_image(rng, n, m, ignored=0.15)
        o = {'boxes': torch.from_numpy(pb).reshape(-1, 4), 'scores': torch.from_numpy(ps), 'labels': torch.from_numpy(pl)}
        t = {'boxes': torch.from_numpy(tb).reshape(-1, 4), 'labels': torch.from_numpy(tl)}
        host.add(o, t)
        mine.add(o, t)
        n_images += 1
        hit, live, match, _ = ref.match_image(pb, ps, pl, tb, tl, mine.iouv, ignore)
        n_pairs += int((match >= 0).sum())
        n_touched += int((live == 0).sum())
    assert n_images >= 40 and n_pairs > 1000 and (n_touched > 20 or not ignore)
    assert_same_stats(mine.ap_per_class(), host.ap_per_class(iouv=torch.linspace(0.5, 0.95, 10), ignore=list(ignore)))


@pytest.mark.parametrize('n,m,kw', [(0, 50, {}), (50, 0, {}), (700, 900, {}), (3000, 2500, dict(tied_scores=True, dup_truths=True)),
                                    (5000, 5000, dict(ignored=0.3))])
def test_binned_form_equals_dense_form(n, m, kw):
    rng = np.random.default_rng(n + m)
    pb, ps, pl, tb, tl = ref.random_image(rng, n, m, side=1500.0, **kw)
    iouv = np.linspace(0.5, 0.95, 10)
    for rows in (False, True):
        prow = rng.permutation(n) if rows else None
        trow = rng.permutation(m) if rows else None
        dense = ref.match_image(pb, ps, pl, tb, tl, iouv, prow=prow, trow=trow)
        binned = ref.match_binned(pb, ps, pl, tb, tl, iouv, prow=prow, trow=trow)
        for a, b, name in zip(dense, binned, ('hit', 'live', 'match', 'match_iou')):
            np.testing.assert_array_equal(a, b, err_msg=name)


def test_tie_rules_of_the_restatement():
    """worked by hand: two truths at the same place (the lower row is kept), two predictions of one score on one truth (the lower row wins)"""
    tb = np.array([[0, 0, 10, 10], [0, 0, 10, 10]], np.float32)
    pb = np.array([[0, 0, 10, 10], [0, 0, 10, 10], [0, 0, 10, 8]], np.float32)
    ps = np.array([0.5, 0.5, 0.9], np.float32)
    one = np.ones(3, np.int64)
    hit, live, match, miou = ref.match_image(pb, ps, one, tb, one[:2], [0.5, 0.9])
    assert match.tolist() == [-1, -1, 0] and hit.tolist() == [0, 0, 1] and live.tolist() == [1, 1, 1] and miou[2] == np.float32(0.8)
    hit, live, match, miou = ref.match_image(pb[:2], ps[:2], one[:2], tb, one[:2], [0.5, 0.9])
    assert match.tolist() == [0, -1] and hit.tolist() == [3, 0]
    hit, live, match, miou = ref.match_image(pb[:2], ps[:2], one[:2], tb, one[:2], [0.5, 0.9], prow=[1, 0], trow=[1, 0])
    assert match.tolist() == [-1, 1] and hit.tolist() == [0, 3]
    # an ignored truth only touches: the prediction leaves the curves
    hit, live, match, miou = ref.match_image(pb[:1], ps[:1], one[:1], tb[:1], np.array([-100]), [0.5])
    assert match.tolist() == [-1] and live.tolist() == [0]


def test_chunk_visit_count_of_the_restatement():
    # two blocks of predictions far apart, two chunks of truths under them: each block meets its own chunk only
    pb = np.concatenate([np.tile([0, 0, 10, 10], (4, 1)), np.tile([100, 100, 110, 110], (4, 1))]).astype(np.float32)
    tb = np.concatenate([np.tile([5, 5, 15, 15], (4, 1)), np.tile([105, 105, 115, 115], (4, 1))]).astype(np.float32)
    off = np.array([0, 8])
    assert ref.chunk_visits(pb, off, tb, off, block=4, chunk=4) == (2, 4)
    assert ref.chunk_visits(pb, off, tb, off, block=8, chunk=4) == (2, 2)
    tb[0, 0] = np.nan                                    # a non-finite truth: its chunk is visited by every block
    assert ref.chunk_visits(pb, off, tb, off, block=4, chunk=4) == (3, 4)
    pb[0, 3] = np.inf                                    # a non-finite prediction: its block visits every chunk
    assert ref.chunk_visits(pb, off, tb, off, block=4, chunk=4) == (4, 4)
    assert ref.chunk_visits(pb, np.array([0, 8, 8]), tb, np.array([0, 0, 8]), block=4, chunk=4) == (0, 0)


# ---- ABI surface: decided on the host, before any launch --------------------------------------------------------------------------------
FAKE = 0x10000      # a 16-byte aligned non-NULL "device pointer", never dereferenced: every call below must fail validation first


@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


def _call(lib, n_iou=10, ws_bytes=None, B=4, NP=1000, NT=2000, pair_iou=0.5, n_ignore=2, **ptrs):
    iouv = (ctypes.c_float * 16)(*np.linspace(0.5, 0.95, 16).tolist())
    ign = (ctypes.c_longlong * 4)(-100, -1, 0, 0)
    need = lib.hdy_ap_match_workspace_bytes(B, NP, NT)
    p = dict(pb=FAKE, ps=FAKE, pl=FAKE, poff=FAKE, prow=None, tb=FAKE, tl=FAKE, toff=FAKE, trow=None, iouv=iouv, ign=ign, hit=FAKE, live=FAKE,
             match=FAKE, miou=FAKE, ws=FAKE)
    p.update(ptrs)
    return lib.hdy_ap_match(p['pb'], p['ps'], p['pl'], p['poff'], p['prow'], NP, p['tb'], p['tl'], p['toff'], p['trow'], NT, B, p['iouv'], n_iou,
                            pair_iou, p['ign'], n_ignore, p['hit'], p['live'], p['match'], p['miou'], p['ws'], need if ws_bytes is None else ws_bytes, None)


def test_abi_workspace_query(lib):
    assert lib.hdy_version() == _lib.ABI_VERSION >= 10
    small, big = lib.hdy_ap_match_workspace_bytes(1, 0, 0), lib.hdy_ap_match_workspace_bytes(64, 19200, 25600)
    assert small >= 64 and small % 16 == 0 and big % 16 == 0
    assert big >= 64 + 25600 * 8 + 2 * 65 * 4                      # header, one claim word per truth, two prefix arrays
    assert big <= 64 + 25600 * 8 + 25600 + 64 * 64                 # ... and little else: chunk boxes, 20 B per 64 truths
    assert lib.hdy_ap_match_workspace_bytes(-1, 0, 0) == 0 and lib.hdy_ap_match_workspace_bytes(1, -5, 0) == 0
    assert lib.hdy_ap_match_workspace_bytes(1, 1 << 30, 0) == 0
    assert lib.hdy_exec_op(b'hdy_ap_match') >= 0


def test_abi_invalid_calls_are_statuses(lib):
    need = lib.hdy_ap_match_workspace_bytes(4, 1000, 2000)
    for name in ('pb', 'ps', 'pl', 'poff', 'tb', 'tl', 'toff', 'hit', 'live', 'match', 'miou', 'iouv'):
        assert _call(lib, **{name: None}) == _lib.EINVAL and b'null' in lib.hdy_last_error(), name
    assert _call(lib, ws=None) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert _call(lib, ws_bytes=need - 16) == _lib.EINVAL and b'workspace' in lib.hdy_last_error()
    assert _call(lib, ws_bytes=0) == _lib.EINVAL
    assert _call(lib, n_iou=0) == _lib.EINVAL and b'n_iou' in lib.hdy_last_error()
    assert _call(lib, n_iou=17) == _lib.EINVAL and b'n_iou' in lib.hdy_last_error()
    assert _call(lib, n_ignore=5) == _lib.EINVAL and _call(lib, n_ignore=-1) == _lib.EINVAL
    assert _call(lib, NP=-1) == _lib.EINVAL and _call(lib, NT=-1) == _lib.EINVAL and _call(lib, B=-1) == _lib.EINVAL
    assert _call(lib, pair_iou=0.0) == _lib.EINVAL and _call(lib, pair_iou=float('nan')) == _lib.EINVAL      # pruning needs a positive bound
    assert _call(lib, pb=FAKE + 4) == _lib.EINVAL and b'aligned' in lib.hdy_last_error()
    assert _call(lib, tl=FAKE + 4) == _lib.EINVAL and _call(lib, match=FAKE + 2) == _lib.EINVAL and _call(lib, ws=FAKE + 8) == _lib.EINVAL
    assert _call(lib, prow=FAKE + 1) == _lib.EINVAL
    with _lib.option('HDY_AP_CHUNK', 100):
        assert _call(lib) == _lib.EINVAL and b'HDY_AP_CHUNK' in lib.hdy_last_error()
