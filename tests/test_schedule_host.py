"""CPU side of the backward-schedule tests (tests/schedule_ref.py): the window rule on hand-made lists, the footprint model (NHWC channel
slices as rows at a pitch, const-ness from include/hdyolo.h, the hdy_stat_req array), the conflict finder on a list with and without the
hazard, and the two extreme one-stream orders.  CPU tensors stand in for device buffers: they have data_ptr() too.  No kernel runs."""
import ctypes
import os

import pytest
import torch

from hd_yolo_amd import _lib, build

import schedule_ref as S


class Side:                                     # stands in for ops.SideStream
    pass


SIDE = Side()


def fork(token, *recs):
    return ('@fork', SIDE, list(recs), token)


def join(token):
    return ('@join', SIDE, token)


def nhwc_buf(c, n=2, h=3, w=5, dtype=torch.bfloat16):
    return torch.zeros(n, h, w, c, dtype=dtype)


# ------------------------------------------------------------------------------------------ windows
def test_windows_follow_list_position_not_token_order():
    a, b, c, d, e = (('hdy_copy_f32', (0, 0, 0), ()) for _ in range(5))
    mark = ('@call', lambda: None)
    #        0           1  2           3  4        5     6  7        8
    recs = [fork(7, a), b, fork(2, a), c, join(7), mark, d, join(2), e]
    # join(7) at 4 covers the fork at 0 only (the fork at 2 is behind it in the list, whatever its token); join(2) covers both
    assert S.windows(recs) == {0: [1, 3], 2: [3, 5, 6]}
    # one closing join of the LAST fork in list order covers everything in front of it
    recs = [fork(5, a), b, fork(0, a), c, fork(3, a), d, join(3)]
    assert S.windows(recs) == {0: [1, 3, 5], 2: [3, 5], 4: [5]}
    # ... a join of the highest token does not, when that fork is not the last one
    with pytest.raises(S.ScheduleError, match=r"'@fork' at 2 .* not covered"):
        S.windows([fork(5, a), b, fork(0, a), c, fork(3, a), d, join(5)])
    assert S.windows([a, b]) == {}


def test_windows_refuse_malformed_lists():
    a = ('hdy_copy_f32', (0, 0, 0), ())
    with pytest.raises(S.ScheduleError, match='not covered'):
        S.windows([fork(0, a), a])
    with pytest.raises(S.ScheduleError, match='names token 4'):
        S.windows([fork(0, a), join(4), join(0)])
    with pytest.raises(S.ScheduleError, match='names token 1'):            # the join sits in front of its fork: it would wait for nothing
        S.windows([fork(0, a), join(1), fork(1, a), join(0)])
    with pytest.raises(S.ScheduleError, match='same token'):
        S.windows([fork(0, a), fork(0, a), join(0)])


# ------------------------------------------------------------------------------------------ regions
def test_channel_slices_are_rows_at_a_pitch():
    buf = nhwc_buf(48)
    es, base = 2, buf.data_ptr()
    full = S.region_of(buf)
    assert (full.rows, full.row, full.lo, full.hi) == (1, 2 * 3 * 5 * 48 * es, base, base + 2 * 3 * 5 * 48 * es)
    a, b, c = buf[..., 0:16], buf[..., 16:48], buf[..., 8:24]
    ra, rb, rc = S.region_of(a), S.region_of(b), S.region_of(c)
    assert (ra.base, ra.rows, ra.row, ra.pitch) == (base, 30, 16 * es, 48 * es)
    assert (rb.base, rb.rows, rb.row, rb.pitch) == (base + 16 * es, 30, 32 * es, 48 * es)
    # interleaved slices of one buffer: their bounding ranges overlap, their bytes do not
    assert ra.lo < rb.hi and rb.lo < ra.hi and not S.overlap(ra, rb) and not S.overlap(rb, ra)
    assert S.overlap(ra, rc) and S.overlap(rc, rb) and S.overlap(rb, rc)
    assert S.overlap(full, ra) and S.overlap(rb, full)
    # touching column ranges: [0, 16) and [16, 48) share no byte, one more channel does
    assert S.overlap(S.region_of(buf[..., 0:17]), rb)
    # a short plain range against rows: inside a column range or in the gap between two rows
    one = torch.zeros(1)
    assert S.overlap(S.Region(base + 48 * es * 7 + 4, 1, 8), ra) and not S.overlap(S.Region(base + 48 * es * 7 + 16 * es, 1, 8), ra)
    assert not S.overlap(S.Region(base - 8, 1, 8), ra) and not S.overlap(S.Region(ra.hi, 1, 8), ra)
    # the last row ends at its column range, not at the pitch
    assert ra.hi == base + 29 * 48 * es + 16 * es and not S.overlap(S.Region(ra.hi, 1, 64), ra)
    # a batch slice of a channel slice keeps the pitch; slices of two pitches fall back to the bounding ranges
    assert S.region_of(buf[1:, :, :, 16:48]).rows == 15
    assert S.overlap(S.Region(base, 30, 32, 64), ra)
    # statistics slabs [tiles][2][K] sliced in K, a 1-D slice, a scalar, an empty tensor, a transposed (non-uniform) view
    slabs = torch.zeros(7, 2, 24)
    r = S.region_of(slabs[:, :, 8:])
    assert (r.rows, r.row, r.pitch) == (14, 16 * 4, 24 * 4)
    assert S.region_of(slabs.view(-1)[5:9]).row == 16 and S.region_of(one).row == 4 and S.region_of(one[:0]).row == 0
    t = torch.zeros(4, 6).t()
    rt = S.region_of(t)
    assert rt.rows == 1 and rt.row == 24 * 4
    assert not S.overlap(S.region_of(one[:0]), S.region_of(one))


def test_overlap_agrees_with_byte_sets_on_random_slices():
    """the row arithmetic against brute force: sets of byte offsets of random channel / batch slices of one buffer"""
    import random
    rng = random.Random(3)
    buf = torch.zeros(3, 2, 4, 20, dtype=torch.int16)
    base = buf.data_ptr()

    def bytes_of(t):
        idx = torch.arange(buf.numel()).view(buf.shape)
        sel = idx[t]
        return {int(i) * 2 + k for i in sel.flatten() for k in (0, 1)}

    for _ in range(300):
        sl = []
        for _ in range(2):
            n0, c0 = rng.randrange(3), rng.randrange(19)
            sl.append((slice(n0, rng.randrange(n0 + 1, 4)), slice(None), slice(None), slice(c0, rng.randrange(c0 + 1, 21))))
        ra, rb = S.region_of(buf[sl[0]]), S.region_of(buf[sl[1]])
        assert ra.lo >= base and S.overlap(ra, rb) == bool(bytes_of(sl[0]) & bytes_of(sl[1])), sl


# ------------------------------------------------------------------------------------------ prototypes and footprints
@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_lib.LIB_PATH):
        build.build(verbose=False)
    return _lib.load()


# what the binding must hold for a type as the header writes it (`const` removed); any pointer but `char*` is c_void_p
SCALAR_KINDS = {'int': ctypes.c_int, 'unsigned': ctypes.c_uint, 'long long': ctypes.c_longlong, 'unsigned long long': ctypes.c_ulonglong,
                'size_t': ctypes.c_size_t, 'float': ctypes.c_float, 'double': ctypes.c_double, 'char*': ctypes.c_char_p, 'void': None}


def kind_of(ctype):
    words = ' '.join(w for w in ctype.replace('*', ' * ').split() if w != 'const').replace(' *', '*')
    return SCALAR_KINDS[words] if words in SCALAR_KINDS else ctypes.c_void_p if words.endswith('*') else words


def test_prototypes_agree_with_the_ctypes_signatures(lib):
    """every function the header declares, read by this file's own reader: the binding's restype and argtypes are the header's types, position
    by position — pointers as c_void_p (c_char_p for strings), every scalar by its own kind"""
    protos, returns = S.prototypes(), S.return_types()
    assert sorted(protos) == sorted(returns) == sorted(_lib.SIGNATURES) and len(protos) >= 110
    assert kind_of('const float* const*') is ctypes.c_void_p and kind_of('const char *') is ctypes.c_char_p and kind_of('short') == 'short'
    for name, params in protos.items():
        restype, types = _lib.SIGNATURES[name]
        assert kind_of(returns[name]) is restype, (name, returns[name])
        assert len(params) == len(types), (name, params)
        assert [p.pointer for p in params] == [t in (ctypes.c_void_p, ctypes.c_char_p) for t in types], (name, params)
        assert [kind_of(p.ctype) for p in params] == types, (name, params)
        assert [(p.name, p.const) for p in params] == _lib.PARAMS[name], name
    listed = [n for n in _lib.SIGNATURES if lib.hdy_exec_op(n.encode()) >= 0]
    assert len(listed) >= 40
    for name in listed:
        params = protos[name]
        assert params[-1].name == 'stream' and not params[-1].const
    # spot checks of what footprint() relies on: names, const-ness, the request array
    w = {p.name: p for p in protos['hdy_conv_wgrad']}
    assert w['x'].const and w['dy'].const and not w['grad_a'].const and not w['workspace'].const and not w['ws_bytes'].pointer
    b = {p.name: p for p in protos['hdy_bn_act_bwd']}
    assert b['dz'].const and not b['dy'].const and not b['dgamma'].const and not b['workspace'].const
    s = {p.name: p for p in protos['hdy_conv_dgrad_stats']}
    assert 'hdy_stat_req' in s['stats'].ctype and s['stats'].pointer and [p.name for p in protos['hdy_conv_dgrad_stats']][-2] == 'nstat'


def wgrad(x, dy, grad, ws):
    return S.record('hdy_conv_wgrad', x=x, ldx=x.shape[3], dy=dy, lddy=dy.stride(2), grad_a=grad, K_a=grad.shape[0], workspace=ws, ws_bytes=ws.numel() * 4)


def bn_bwd(dz, y, dy, dgamma, dbeta, ws):
    return S.record('hdy_bn_act_bwd', dz=dz, lddz=dz.stride(2), y=y, ldy=y.stride(2), dy=dy, lddy=0 if dy is None else dy.stride(2),
                    dgamma=dgamma, dbeta=dbeta, workspace=ws, ws_bytes=ws.numel() * 4)


def test_footprint_reads_extent_from_the_tensors_and_direction_from_the_header():
    x, ring, grad, ws = nhwc_buf(8), nhwc_buf(32), torch.zeros(16, 8, 3, 3), torch.zeros(100)
    dy = ring[..., 16:32]
    fp = {a.arg: a for a in S.footprint(wgrad(x, dy, grad, ws))}
    assert sorted(fp) == ['dy', 'grad_a', 'workspace', 'x']                 # grad_b is NULL: no entry
    assert not fp['x'].write and not fp['dy'].write and fp['grad_a'].write and fp['workspace'].write
    assert fp['dy'].region == S.region_of(dy) and fp['dy'].region.rows == 30 and fp['workspace'].region.row == 400
    # a non-null pointer nobody keeps is an error, never a skipped argument
    rec = wgrad(x, dy, grad, ws)
    with pytest.raises(S.ScheduleError, match=r'hdy_conv_wgrad\[workspace\]'):
        S.footprint((rec[0], rec[1], tuple(t for t in rec[2] if t is not ws)))
    with pytest.raises(S.ScheduleError, match='arguments recorded'):
        S.footprint((rec[0], rec[1][:-1], rec[2]))
    with pytest.raises(S.ScheduleError, match='not declared'):
        S.footprint(('hdy_no_such_entry', (), ()))
    # an interior pointer (hdy_bn_finalize_sums' `sums + k0`, `sums + 2 * Ktot`): from there to the end of the tensor that holds it
    sums = torch.zeros(2 * 8 + 1, dtype=torch.float64)
    scale = torch.zeros(8)
    rec = S.record('hdy_bn_finalize_sums', sums=sums.data_ptr() + 8 * 4, count=sums.data_ptr() + 16 * 8, scale=scale)
    fp = {a.arg: a for a in S.footprint((rec[0], rec[1], (sums, scale)))}
    assert fp['sums'].region == S.Region(sums.data_ptr() + 32, 1, 17 * 8 - 32) and not fp['sums'].write and fp['scale'].write
    assert fp['count'].region.row == 8


def test_footprint_of_a_statistics_request_array():
    """hdy_conv_dgrad_stats as ops.rec_conv_dgrad builds it: the request array rides behind the kept tensors; slabs written, y / scale / shift read"""
    dy, dx, wp = nhwc_buf(16), nhwc_buf(24), torch.zeros(16 * 24, dtype=torch.bfloat16)
    yraw, scale, shift = nhwc_buf(40), torch.zeros(40), torch.zeros(40)
    reqs = []
    for k0, K, c0 in ((0, 16, 0), (16, 8, 16)):
        y, slabs = yraw[..., k0:k0 + K], torch.zeros(3, 2, K)
        reqs.append((_lib.StatReq(y.data_ptr(), 40, scale[k0:].data_ptr(), shift[k0:].data_ptr(), slabs.data_ptr(), c0, c0 + K, 1, 3),
                     (y, scale[k0:k0 + K], shift[k0:k0 + K], slabs)))
    arr = (_lib.StatReq * 2)(*[q for q, _ in reqs])
    rec = S.record('hdy_conv_dgrad_stats', dy=dy, lddy=16, w_packed_dgrad=wp, dx=dx, lddx=24, nstat=2)
    args = list(rec[1])
    args[[p.name for p in S.prototypes()[rec[0]]].index('stats')] = ctypes.cast(arr, ctypes.c_void_p)
    rec = (rec[0], tuple(args), rec[2] + tuple(t for _, keep in reqs for t in keep), (arr,))
    fp = {a.arg: a for a in S.footprint(rec)}
    assert {k for k in fp if k.startswith('stats')} == {f'stats[{i}].{f}' for i in (0, 1) for f in ('y', 'scale', 'shift', 'slabs')}
    assert fp['stats[1].slabs'].write and not fp['stats[1].y'].write and not fp['stats[0].scale'].write and fp['dx'].write and not fp['dy'].write
    assert fp['stats[1].y'].region == S.region_of(yraw[..., 16:24]) and fp['stats[0].slabs'].region.row == 3 * 2 * 16 * 4
    with pytest.raises(S.ScheduleError, match='request array'):
        S.footprint(rec[:3])


# ------------------------------------------------------------------------------------------ conflicts
def ring_list(joined):
    """two layers of a backward list over a ONE-slot dy ring: BatchNorm backward writes dy, the weight gradient (forked) reads it"""
    x, ring, bn_ws, wg_ws = nhwc_buf(8), torch.zeros(2 * 3 * 5 * 16, dtype=torch.bfloat16), torch.zeros(64), torch.zeros(100)
    dz, y = nhwc_buf(16), nhwc_buf(16)
    g1, g2, dg, db = torch.zeros(16, 8, 3, 3), torch.zeros(16, 8, 3, 3), torch.zeros(16), torch.zeros(16)
    dy = ring.view(2, 3, 5, 16)
    recs = [bn_bwd(dz, y, dy, dg, db, bn_ws), fork(0, wgrad(x, dy, g1, wg_ws))]
    if joined:
        recs.append(join(0))
    recs += [bn_bwd(dz, y, dy, dg, db, bn_ws), fork(1, wgrad(x, dy, g2, wg_ws)), join(1)]
    return recs, ring


def test_conflicts_find_the_missing_join_and_nothing_else():
    recs, ring = ring_list(joined=True)
    assert S.conflicts(recs) == []
    recs, ring = ring_list(joined=False)
    found = S.conflicts(recs)
    assert len(found) == 1
    c = found[0]
    assert (c.fork_pos, c.fork_symbol, c.fork_arg, c.fork_write) == (1, 'hdy_conv_wgrad', 'dy', False)
    assert (c.main_pos, c.main_symbol, c.main_arg, c.main_write) == (2, 'hdy_bn_act_bwd', 'dy', True)
    assert c.fork_region.inside(ring) and "no '@join' between 1 and 2" in repr(c) and 'hdy_conv_wgrad' in repr(c) and '`dy`' in repr(c)
    # two readers never conflict; a main-stream launch sharing the side stream's workspace does (two writers)
    x, dy, ws = nhwc_buf(8), nhwc_buf(16), torch.zeros(100)
    ga, gb = torch.zeros(16, 8, 3, 3), torch.zeros(16, 8, 3, 3)
    assert S.conflicts([fork(0, wgrad(x, dy, ga, ws)), wgrad(x, dy, gb, torch.zeros(100)), join(0)]) == []
    found = S.conflicts([fork(0, wgrad(x, dy, ga, ws)), wgrad(x, dy, gb, ws), join(0)])
    assert [(c.fork_arg, c.main_arg) for c in found] == [('workspace', 'workspace')] and found[0].fork_region.inside(ws)
    # interleaved channel slices of one buffer behind a fork: no conflict; one channel of overlap: conflict
    wide = nhwc_buf(32)
    left = bn_bwd(nhwc_buf(16), nhwc_buf(16), wide[..., :16], torch.zeros(16), torch.zeros(16), torch.zeros(64))
    assert S.conflicts([fork(0, wgrad(x, wide[..., 16:], ga, ws)), left, join(0)]) == []
    found = S.conflicts([fork(0, wgrad(x, wide[..., 15:31], ga, ws)), left, join(0)])
    assert [(c.fork_arg, c.main_arg, c.main_write) for c in found] == [('dy', 'dy', True)]
    # the window ends at the covering join: the same writer behind it is fine
    assert S.conflicts([fork(0, wgrad(x, wide[..., 15:31], ga, ws)), join(0), left]) == []


def test_early_marks_sees_a_writer_behind_the_mark():
    flat = torch.zeros(64)
    x, dy, ws = nhwc_buf(8), nhwc_buf(16), torch.zeros(100)
    ga = flat[16:16 + 8 * 2].view(2, 8, 1, 1)
    src = torch.zeros(4)

    def mark(a, b):
        fn = lambda: None
        fn.hdy_mark = (a, b)
        return ('@call', fn)

    copy = S.record('hdy_copy_f32', src=src, dst=flat[40:44], n=4)
    good = [copy, fork(0, wgrad(x, dy, ga, ws)), mark(16, 64), S.record('hdy_copy_f32', src=src, dst=flat[4:8], n=4), mark(0, 16), join(0)]
    assert S.early_marks(good, flat) == []
    bad = [copy, mark(16, 64), fork(0, wgrad(x, dy, ga, ws)), mark(0, 16), join(0)]           # the forked writer of [16, 32) sits behind its mark
    found = S.early_marks(bad, flat)
    assert [(p, r) for p, r, _ in found] == [(1, (16, 64))] and found[0][2] == [(2, 'hdy_conv_wgrad', 'grad_a')]
    assert S.writers(bad, flat.data_ptr() + 40 * 4, flat.data_ptr() + 41 * 4) == [(0, 'hdy_copy_f32', 'dst')]


# ------------------------------------------------------------------------------------------ canonical form
def canon_list(dy_off=16, first='hdy_bn_act_bwd', second_forked=True, join_at=4):
    """one small two-stream list over FRESH allocations: BatchNorm backward into a channel slice of a wide buffer, two forked weight gradients
    (one fed by a data gradient that serves a statistics request), a mark, a host call, the join"""
    x, wide, bn_ws, wg_ws, flat = nhwc_buf(8), nhwc_buf(48), torch.zeros(64), torch.zeros(100), torch.zeros(2 * 16 * 8 * 9 + 32)
    dz, y, dx, wp, scale = nhwc_buf(16), nhwc_buf(16), nhwc_buf(8), torch.zeros(16 * 8, dtype=torch.bfloat16), torch.zeros(16)
    g1, g2, dg, db = flat[:1152].view(16, 8, 3, 3), flat[1152:2304].view(16, 8, 3, 3), flat[2304:2320], flat[2320:]
    dy = wide[..., dy_off:dy_off + 16]
    a = bn_bwd(dz, y, dy, dg, db, bn_ws) if first == 'hdy_bn_act_bwd' else S.record(first, src=dg, dst=db, n=16)
    slabs = torch.zeros(3, 2, 8)
    arr = (_lib.StatReq * 1)(_lib.StatReq(y[..., 8:].data_ptr(), 16, scale[8:].data_ptr(), None, slabs.data_ptr(), 0, 8, 1, 3))
    d = S.record('hdy_conv_dgrad_stats', dy=dy, lddy=48, w_packed_dgrad=wp, dx=dx, lddx=8, nstat=1)
    args = list(d[1])
    args[[p.name for p in S.prototypes()[d[0]]].index('stats')] = ctypes.cast(arr, ctypes.c_void_p)
    d = (d[0], tuple(args), d[2] + (y[..., 8:], scale[8:], slabs), (arr,))
    mark = lambda: None
    mark.hdy_mark = (1152, 2304)
    w1, w2 = wgrad(x, dy, g1, wg_ws), wgrad(dx, dy, g2, wg_ws)
    recs = [a, d, fork(0, w1, w2) if second_forked else fork(0, w1), ('@call', mark), ('@call', lambda: None)]
    if not second_forked:
        recs.insert(3, w2)
    recs.insert(join_at, join(0))
    return recs


def test_canonical_form_is_free_of_addresses_and_sees_every_change():
    base = S.canonical(canon_list())
    assert base == S.canonical(canon_list())                    # same structure, other allocations
    kinds = [r[0] for r in base]
    assert kinds == ['hdy_bn_act_bwd', 'hdy_conv_dgrad_stats', '@fork', '@call', '@join', '@call']
    assert base[3] == ('@call', (1152, 2304)) and base[5] == ('@call', 'host') and base[4] == ('@join', 0) and base[2][1] == 0
    # storages are numbered as they first appear (dz, y, the wide buffer ...); a channel slice keeps its offset and its rows at the pitch
    bn = dict(zip([p.name for p in S.prototypes()['hdy_bn_act_bwd']], base[0][1]))
    assert bn['dz'] == (0, 0, 1, 30 * 16 * 2, 30 * 16 * 2) and bn['y'][0] == 1 and bn['dy'] == (2, 16 * 2, 30, 16 * 2, 48 * 2) and bn['mean'] is None
    assert bn['lddy'] == 48 and bn['dbeta'][:2] == (bn['dgamma'][0], bn['dgamma'][1] + 64)
    # both forked weight gradients write one flat buffer at their offsets, and read the dy the first record wrote
    w1, w2 = (dict(zip([p.name for p in S.prototypes()['hdy_conv_wgrad']], q[1])) for q in base[2][2])
    assert w1['grad_a'][:2] == (bn['dgamma'][0], 0) and w2['grad_a'][:2] == (bn['dgamma'][0], 1152 * 4) and w1['dy'] == w2['dy'] == bn['dy']
    # the request array, field by field: y is a slice of the second storage, the null shift stays None, scalars verbatim
    req, = dict(zip([p.name for p in S.prototypes()['hdy_conv_dgrad_stats']], base[1][1]))['stats']
    assert req[0] == (1, 8 * 2, 30, 8 * 2, 16 * 2) and req[1] == 16 and req[2][1] == 8 * 4 and req[3] is None and req[5:] == (0, 8, 1, 3)
    for other in (canon_list(dy_off=24),                        # a changed offset
                  canon_list(first='hdy_copy_f32'),             # a changed symbol
                  canon_list(second_forked=False),              # a record moved from the fork to the main list
                  canon_list(join_at=3)):                       # a moved join
        assert S.canonical(other) != base
    # a pointer that no kept tensor accounts for is an error here too
    recs = canon_list()
    recs[0] = (recs[0][0], recs[0][1], recs[0][2][1:])
    with pytest.raises(S.ScheduleError, match=r'hdy_bn_act_bwd\[dz\]'):
        S.canonical(recs)


# ------------------------------------------------------------------------------------------ the two extreme orders
def drive(recs, log):
    """ops.run's dispatch without a device: launch records are logged instead of launched"""
    for rec in recs:
        if rec[0] == '@call':
            rec[1]()
        elif rec[0] == '@fork':
            rec[1].fork(rec[2], rec[3], None)
        elif rec[0] == '@join':
            rec[1].join(rec[2], None)
        else:
            log.append(rec[0])


def test_early_and_late_orders():
    A, B, C, D, W0, W1, W2 = ((n, (), ()) for n in ('A', 'B', 'C', 'D', 'w0', 'w1', 'w2'))

    class P:
        bucket_hook = None
    plan = P()
    seen = []
    fn = lambda: plan.bucket_hook(0, 4, None) if plan.bucket_hook else None
    recs = [A, fork(5, W0), B, fork(1, W1), ('@call', fn), C, join(5), fork(3, W2), D, join(3)]
    log = []
    run = lambda records: drive(records, log)
    with S.early(SIDE, run=run):
        drive(recs, log)
    assert log == ['A', 'w0', 'B', 'w1', 'C', 'w2', 'D'] and 'fork' not in SIDE.__dict__ and 'join' not in SIDE.__dict__
    del log[:]
    with S.late(SIDE, run=run):
        drive(recs, log)
    assert log == ['A', 'B', 'C', 'w0', 'D', 'w1', 'w2']          # join(5) runs the fork at 1 only; w1 waits for join(3), in order before w2
    # with a bucket hook installed, a mark flushes what is queued (the hook's consumer waits for the side stream)
    plan.bucket_hook = lambda a, b, s: seen.append((a, b, list(log)))
    del log[:]
    with S.late(SIDE, plan=plan, run=run):
        drive(recs, log)
    assert log == ['A', 'B', 'w0', 'w1', 'C', 'D', 'w2'] and seen == [(0, 4, ['A', 'B', 'w0', 'w1'])]
    assert plan.bucket_hook is not None and plan.bucket_hook.__name__ == '<lambda>'
    # a list that ends with forks still queued is malformed
    with pytest.raises(S.ScheduleError, match='never joined'):
        with S.late(SIDE, run=run):
            drive([A, fork(0, W0), B], log)
    assert 'fork' not in SIDE.__dict__
