"""The two-stream backward schedule (Plan._compile_backward: weight gradients forked onto a side stream, joins placed by hand-made rules)
on a real MI355X, with the host-side model of tests/schedule_ref.py.

A missing join is a data race, and a race shows only when the timing exposes it: the golden and repeat tests pass on most runs with one.
Three checks here do not depend on timing:

  a. static      schedule_ref.conflicts(plan.bwd) == []: no forked record shares bytes, one side writing, with a main-stream record that may
                 run beside it.  This is the ONLY check that sees two concurrent launches sharing scratch (the inline weight gradients'
                 second workspace, HDY_FORK_MIN_PIXELS > 0): a serial order runs them one after the other and computes the right numbers.
  b. marks       no record at or behind a "gradient range [a, b) is final" mark may write into that range (from the footprints, not from
                 the plan's own log).
  c. orders      one full step (forward, fused loss, backward; no optimizer step) three times from the same weights, tiles and targets: the
                 real two-stream run through the compiled Program, and the list on ONE stream in its two extreme legal orders — every fork
                 run at its fork point (early), every fork held back to the first join that covers it (late).  Every two-stream execution
                 lies between the two; a read-after-write, write-after-read or write-after-write hazard between a forked record and a
                 record in its window gives them different inputs, deterministically.  All gradients must agree bit for bit: the kernels
                 are deterministic (tests/test_gpu_scratch.py::test_repeats_are_bit_identical relies on the same), no tolerance is involved.

over the knobs nothing else in the suite moves: HDY_DY_RING 1 / 2 / 4, HDY_FORK_MIN_PIXELS, HDY_PRODUCER_STATS, small gradient buckets, a
frozen backbone, SyncBatchNorm lists (static only).  Two negative controls show that the checks can fail: the ring's joins deleted (a and c
see it), the two weight-gradient workspaces made one (a sees it).

The forward list of the same plans is checked as a list: every ConvUnit's records are the sequence its Plan._bn_fwd_mode stands for, every
pointer is covered by a tensor its record keeps alive (what makes replaying a stored list safe), and compiling again gives the same list.

The mask branch is left out (compute_masks=False): roi_align's backward scatters with global atomics and is not bit-reproducible from run to
run; its records hold no forks.  The engines here carry no bucket hooks (single process), so a mark does not wait for the side stream and the
late order does not flush at marks; schedule_ref.late(side, plan) does, and tests/test_schedule_host.py covers that."""
import collections
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from hd_yolo_amd import ops, synth  # noqa: E402
from hd_yolo_amd import plan as planmod  # noqa: E402

import schedule_ref as S  # noqa: E402

DEV = 'cuda:0'
F32, BF16 = torch.float32, torch.bfloat16

# geometry: variant, tile side, classes, boxes per tile (the train_* goldens' of tests/test_gpu_model.py), arithmetic type, first tile without targets
GEOM = {
    'n64-fp32': ('n', 64, 2, (3, 8), F32, False),
    's128-bf16': ('s', 128, 8, (10, 30), BF16, False),
    'm128-bf16': ('m', 128, 8, (10, 30), BF16, False),
    'n64-ragged': ('n', 64, 2, (3, 8), F32, True),
}
BATCH = 2
# HDY_FORK_MIN_PIXELS between the smallest and the largest layer: output pixels per layer are 8 ... 2048 (64x64 tiles), 32 ... 8192 (128x128).
# The stride-8 level and everything finer forks, the two coarse levels run inline: the neck walks up and down the levels, so inline weight
# gradients sit inside the windows of forked ones (a threshold above the stride-8 level would leave every fork at the end of the list)
FORK_MIN = {64: 100, 128: 200}
SMALL_BUCKETS = 256 << 10

Case = collections.namedtuple('Case', 'geom ring fork_min prod buckets frozen sync', defaults=(4, False, 'fused', False, False, False))


def case_id(c):
    return '-'.join([c.geom, f'ring{c.ring}'] + (['forkmin'] if c.fork_min else []) + ([f'prod_{c.prod}'] if GEOM[c.geom][4] == BF16 else []) +
                    (['buckets'] if c.buckets else []) + (['frozen'] if c.frozen else []) + (['syncbn'] if c.sync else []))


# the cross product pruned to what is distinct: every ring size with and without inline weight gradients, every statistics mode on both bf16
# models, small buckets on the list with the most parameters per launch, the frozen list at both ends of the ring
CASES = [
    Case('n64-fp32'), Case('n64-fp32', ring=1), Case('n64-fp32', ring=2), Case('n64-fp32', fork_min=True), Case('n64-fp32', ring=1, fork_min=True),
    Case('n64-fp32', buckets=True), Case('n64-fp32', ring=2, fork_min=True, buckets=True), Case('n64-fp32', frozen=True), Case('n64-fp32', ring=1, frozen=True),
    Case('s128-bf16'), Case('s128-bf16', prod='1'), Case('s128-bf16', prod='0'), Case('s128-bf16', ring=1), Case('s128-bf16', ring=2, fork_min=True, prod='1'),
    Case('s128-bf16', ring=1, fork_min=True, prod='0'), Case('s128-bf16', ring=1, prod='1', buckets=True),
    Case('m128-bf16'), Case('m128-bf16', ring=1, prod='1'), Case('m128-bf16', ring=2, fork_min=True, prod='0'),
    Case('n64-ragged'), Case('n64-ragged', ring=1, fork_min=True),
]
SYNC_CASES = [Case('n64-fp32', ring=1, sync=True), Case('n64-fp32', fork_min=True, buckets=True, sync=True), Case('s128-bf16', ring=2, sync=True)]


class Built:
    def __init__(self, case):
        from metayolo.models.yolo import Model
        self.case = case
        variant, self.size, self.nc, self.boxes, self.dtype, self.ragged = GEOM[case.geom]
        with self.knobs():
            model = Model(synth.make_cfg(variant, self.nc), synth.make_hyp())
            sd = synth.synth_state_dict(synth.shapes_of(model), seed=0)
            assert not model.load_state_dict(sd, strict=False).unexpected_keys
            model = model.to(DEV)
            if case.frozen:
                model.freeze(['backbone', 'neck.0'])
            self.model = model.train()
            self.eng = model._eng()
            if case.sync:
                self.eng.sync_bn = True             # the list is only inspected: building it needs no process group
            self.plan = self.eng.plan_for_shape((BATCH, 3, self.size, self.size), torch.device(DEV), True, self.dtype)
        self.side = next(r[1] for r in self.plan.bwd if r[0] == '@fork')
        self.x = synth.synth_images(BATCH, self.size, seed=11).to(DEV)

    @contextlib.contextmanager
    def knobs(self):
        """the knobs are module attributes read while a plan is built (buffers in _allocate, joins and marks in _compile_backward)"""
        case = self.case
        with pytest.MonkeyPatch.context() as mp:
            for k, v in (('USE_GRAPHS', False), ('SIDE_WGRAD', True), ('STEM_FUSED', True), ('FUSED_1X1', True), ('SKIP_WGRAD', False),
                         ('DY_RING', case.ring), ('FORK_MIN_PIXELS', FORK_MIN[self.size] if case.fork_min else 0), ('PRODUCER_STATS', case.prod)):
                mp.setattr(planmod, k, v)
            if case.buckets:
                mp.setattr(planmod, 'GRAD_BUCKET_BYTES', SMALL_BUCKETS)
            yield

    def rebuilt_backward(self):
        """the backward list compiled again, under the same knobs, from the plan as it stands now (the pack table's entries, which compiling
        appends to, put back)"""
        packs = self.plan.packs
        saved = (list(packs.descs), packs.blocks, list(packs.keep), packs.table)
        try:
            with self.knobs():
                return self.plan._compile_backward()
        finally:
            packs.descs, packs.blocks, packs.keep, packs.table = saved

    def rebuilt_forward(self):
        """the forward list compiled again from the plan as it stands now (the pack table's and the BN-eval table's entries, which compiling
        appends to, put back)"""
        packs, bn = self.plan.packs, self.plan.bn_eval
        saved = (list(packs.descs), packs.blocks, list(packs.keep), packs.table), (list(bn.descs), list(bn.keep), bn.table)
        try:
            with self.knobs():
                return self.plan._compile_forward()
        finally:
            (packs.descs, packs.blocks, packs.keep, packs.table), (bn.descs, bn.keep, bn.table) = saved

    def targets(self):
        t = synth.synth_targets(BATCH, self.size, self.nc, nmin=self.boxes[0], nmax=self.boxes[1], seed=5)       # the model clamps them in place: fresh every step
        if self.ragged:
            a = t[0]['anns']['det'][0]
            a['boxes'], a['labels'] = a['boxes'][:0], a['labels'][:0]
        return t

    def step(self):
        """forward + fused loss + backward from the current weights: {parameter name: gradient copy}"""
        self.model.zero_grad(set_to_none=True)
        auto = torch.autocast('cuda', dtype=BF16) if self.dtype == BF16 else contextlib.nullcontext()
        with auto:
            losses, _ = self.model(self.x, self.targets())
        assert self.eng.last_plan is self.plan and self.plan.loss_call is not None, 'the step ran another plan, or not the fused loss'
        losses['det']['det_loss'].backward()
        torch.cuda.synchronize()
        return {k: p.grad.clone() for k, p in self.model.named_parameters() if p.grad is not None}


@pytest.fixture(scope='module', params=CASES, ids=case_id)
def built(request):
    return Built(request.param)


def arg(rec, name):
    return rec[1][[p.name for p in S.prototypes()[rec[0]]].index(name)]


def split(recs):
    """(main-stream launch records, forked launch records)"""
    return [r for r in recs if r[0][0] != '@'], [q for r in recs if r[0] == '@fork' for q in r[2]]


def check_contents(b):
    """each configuration holds the launches it is there for"""
    case, plan = b.case, b.plan
    inline, forked = split(plan.bwd)
    names = {r[0] for r in inline + forked}
    conv_units = [u for u in plan.units if type(u).__name__ == 'ConvUnit']
    assert forked and plan.bwd[-1][0] == '@join'
    if case.geom in ('n64-fp32', 'n64-ragged'):
        if case.sync:
            assert any(r[0] == 'hdy_bn_act_bwd_apply' for r in inline)
        else:
            assert any(r[0] in ('hdy_bn_act_bwd', 'hdy_bn_act_bwd_pair') and arg(r, 'dy') for r in inline), 'no three-launch BatchNorm backward writing dy'
        assert not any(n.startswith('hdy_conv1x1_bwd_fused') for n in names)
    if case.geom == 's128-bf16' and not case.sync:
        assert any(n.startswith('hdy_conv1x1_bwd_fused') for n in names)
        assert any(r[0] == 'hdy_conv_wgrad_stem_fused' for r in forked), 'the 64x64 stem output meets the 16x32 rule: its fused weight gradient is forked'
        assert (plan.producer_stat_units > 0) == (case.prod != '0'), plan.producer_stat_units
        assert any(n.endswith('_stats') for n in names) == (case.prod != '0')
    if b.dtype == BF16 and case.prod == '0':
        assert plan.producer_stat_units == 0 and not any(n.endswith('_stats') for n in names)
    if case.geom == 'm128-bf16':
        assert {48, 96, 192} <= {u.K for u in conv_units}
    if case.geom == 'n64-ragged':
        t = b.targets()
        assert t[0]['anns']['det'][0]['boxes'].shape[0] == 0 and t[1]['anns']['det'][0]['boxes'].shape[0] > 0
    if case.ring in (1, 2):
        assert len(plan.dy_ring) == case.ring and any(r[0] == '@join' for r in plan.bwd[:-1]), 'a short ring needs joins inside the list'
    if case.fork_min:
        assert any(r[0] == 'hdy_conv_wgrad' for r in inline) and any(r[0] == 'hdy_conv_wgrad' for r in forked)
        assert plan.wg_ws_main is not plan.wg_ws
    else:
        assert plan.wg_ws_main is plan.wg_ws and not any(r[0] == 'hdy_conv_wgrad' for r in inline)
    if case.buckets:
        assert len(plan.bucket_marks()) >= 4, plan.bucket_marks()
    if case.frozen:
        n_conv = sum(1 for u in plan.units if type(u).__name__ in ('ConvUnit', 'DetUnit'))
        assert len(forked) < n_conv - 20
        assert not any(arg(r, 'stem') for r in forked if r[0] == 'hdy_conv_wgrad'), 'a frozen stem has no weight gradient: the list ends elsewhere'
    elif case.geom != 's128-bf16' or case.sync:
        assert arg(forked[-1], 'stem') == 1, 'the stem weight gradient is the last fork'


def assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    bad = [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    assert not bad, f'{what}: {len(bad)} of {len(a)} gradients differ, first {bad[:6]}'


# ------------------------------------------------------------------------------------------ a. static
def test_no_forked_record_races_with_its_window(built):
    check_contents(built)
    found = S.conflicts(built.plan.bwd)
    assert found == [], '\n'.join(map(repr, found[:10]))


@pytest.mark.parametrize('case', SYNC_CASES, ids=case_id)
def test_sync_batchnorm_lists_are_race_free(case):
    """SyncBatchNorm plans take another BatchNorm-backward path (local statistics, all-reduce, apply) and fuse nothing: static check only"""
    b = Built(case)
    assert any(r[0] == 'hdy_bn_bwd_coeffs_sums' for r in b.plan.bwd) and sum(1 for r in b.plan.bwd if r[0] == '@call') > len(b.plan.bucket_marks())
    check_contents(b)
    found = S.conflicts(b.plan.bwd)
    assert found == [], '\n'.join(map(repr, found[:10]))
    assert S.early_marks(b.plan.bwd, b.eng.store.cur) == []


# ------------------------------------------------------------------------------------------ the forward list
UNIT_HEADS = ('hdy_conv_fwd', 'hdy_sppf_pool_fwd', 'hdy_upsample2x_fwd')      # every unit's first forward record, and no other record of a unit
COEFFS = {'single': 'hdy_bn_finalize', 'frozen': 'hdy_bn_eval_coeffs', 'sync': 'hdy_bn_finalize_sums'}
FWD_SEEN = {}                                   # case id -> {(mode, apply symbol)} of the plans checked so far


def forward_symbols(mode, u):
    """the symbols Plan._bn_fwd_mode's answer stands for: the convolution, then the coefficients and the apply pass — one pass over both
    halves when two live modules share the raw tensor and nothing is added, else one per module behind that module's coefficients"""
    n = len(u.mods)
    if mode == 'pair':
        return ['hdy_conv_fwd', 'hdy_bn_finalize_pair', 'hdy_bn_act_fwd_pair']
    head = ['hdy_conv_fwd'] + (['hdy_bn_slab_sums', '@call'] if mode == 'sync' else [])
    if mode == 'sync' and n == 2 and u.res is None:
        return head + [COEFFS[mode]] * n + ['hdy_bn_act_fwd_pair']
    return head + [COEFFS[mode], 'hdy_bn_act_fwd'] * n


def check_forward_modes(b):
    plan = b.plan
    starts = [i for i, r in enumerate(plan.fwd) if r[0] in UNIT_HEADS]
    assert len(starts) == len(plan.units) and starts[0] == 0
    seen = set()
    for u, i, j in zip(plan.units, starts, starts[1:] + [len(plan.fwd)]):
        if type(u).__name__ != 'ConvUnit':
            continue
        assert arg(plan.fwd[i], 'y') == u.yraw.data_ptr(), 'not this unit\'s convolution'
        mode, got = plan._bn_fwd_mode(u), [r[0] for r in plan.fwd[i:j]]
        assert (mode == 'frozen') == u.frozen and (mode == 'sync') == (b.case.sync and not u.frozen), (mode, u.frozen)
        assert mode != 'pair' or (len(u.mods) == 2 and u.res is None)
        assert got == forward_symbols(mode, u), (mode, got)
        seen.add((mode, got[-1]))
    FWD_SEEN[case_id(b.case)] = seen
    S.canonical(plan.fwd)                       # raises for a pointer that no tensor the record keeps alive covers


def test_forward_records_follow_the_mode(built):
    check_forward_modes(built)


@pytest.mark.parametrize('case', SYNC_CASES, ids=case_id)
def test_forward_records_follow_the_mode_with_sync_batchnorm(case):
    check_forward_modes(Built(case))


def test_every_forward_mode_and_both_pair_applies_occur():
    for case in CASES + SYNC_CASES:             # (the two tests above have been over all of them when the whole module runs)
        if case_id(case) not in FWD_SEEN:
            check_forward_modes(Built(case))
    seen = set().union(*(FWD_SEEN[case_id(c)] for c in CASES + SYNC_CASES))
    assert {m for m, _ in seen} == {'sync', 'pair', 'single', 'frozen'}, seen
    assert ('pair', 'hdy_bn_act_fwd_pair') in seen and ('sync', 'hdy_bn_act_fwd_pair') in seen, seen


def test_every_forward_pointer_is_accounted_for(built):
    assert len(S.canonical(built.plan.fwd)) == len(built.plan.fwd)


def test_compiling_the_forward_again_changes_nothing(built):
    """every case: an fp32 and two bf16 models among them"""
    plan = built.plan
    packs, bn_eval = len(plan.packs.descs), len(plan.bn_eval.descs)
    again = built.rebuilt_forward()
    assert again is not plan.fwd and S.canonical(again) == S.canonical(plan.fwd)
    assert (len(plan.packs.descs), len(plan.bn_eval.descs)) == (packs, bn_eval)


# ------------------------------------------------------------------------------------------ b. marks
def test_marks_are_never_early(built):
    plan, flat = built.plan, built.eng.store.cur
    marks = plan.bucket_marks()
    assert marks and min(a for a, _ in marks) == 0 and max(b for _, b in marks) == flat.numel()
    # every trainable gradient has a writer in the list (so the check below looks at something)
    assert S.writers(plan.bwd, flat.data_ptr(), flat.data_ptr() + 4 * flat.numel())
    bad = S.early_marks(plan.bwd, flat)
    assert bad == [], bad[:4]


# ------------------------------------------------------------------------------------------ c. extreme orders
def test_two_streams_and_both_extreme_orders_agree_bitwise(built, monkeypatch):
    b = built
    monkeypatch.setattr(ops, 'USE_EXEC', True)
    real = b.step()
    assert b.plan._progs['bwd'].side is b.side and b.plan._progs['bwd'].records is b.plan.bwd, 'the real run did not go through the compiled two-stream Program'
    monkeypatch.setattr(ops, 'USE_EXEC', False)
    with S.early(b.side):
        first = b.step()
    with S.late(b.side) as order:
        last = b.step()
    assert not order.queue
    conv_w = [k for k in real if k.endswith('conv.weight')]
    assert len(conv_w) >= 10 and all(real[k].abs().max() > 0 for k in conv_w[-3:])
    assert_same_bits(first, last, 'earliest against latest legal order')
    assert_same_bits(real, first, 'two-stream run against the earliest order')


# ------------------------------------------------------------------------------------------ d. negative controls
def test_control_deleted_ring_joins_are_seen_statically_and_by_the_orders(monkeypatch):
    b = Built(Case('n64-fp32', ring=1))
    plan = b.plan
    assert S.conflicts(plan.bwd) == []
    n = len(plan.bwd)
    plan.bwd[:] = [r for i, r in enumerate(plan.bwd) if r[0] != '@join' or i == n - 1]
    assert len(plan.bwd) < n - 10
    found = S.conflicts(plan.bwd)
    ring = [c for c in found if c.fork_symbol == 'hdy_conv_wgrad' and c.fork_arg == 'dy' and not c.fork_write and c.main_symbol.startswith('hdy_bn_act_bwd')
            and c.main_arg == 'dy' and c.main_write and c.fork_region.inside(plan.dy_ring[0]) and c.main_region.inside(plan.dy_ring[0])]
    assert ring, found[:5]
    assert "no '@join' between" in repr(ring[0])
    # on one stream a wrong order gives wrong numbers, never a fault: every read stays inside the ring slot
    monkeypatch.setattr(ops, 'USE_EXEC', False)
    with S.early(b.side):
        first = b.step()
    with S.late(b.side):
        last = b.step()
    differ = [k for k in first if k.endswith('conv.weight') and not torch.equal(first[k].view(torch.int32), last[k].view(torch.int32))]
    assert differ, 'the latest order read every dy after its ring slot was rewritten, and no weight gradient noticed'
    # everything the main stream alone computes is untouched
    same = [k for k in first if not k.endswith('conv.weight') and 'headers' not in k]
    assert same and all(torch.equal(first[k].view(torch.int32), last[k].view(torch.int32)) for k in same)


def test_control_shared_weight_gradient_workspace_is_seen_statically():
    """inline and forked weight gradients on ONE split-slab workspace: two launches that may run at the same time write the same scratch.
    Only the static check can see this one: any serial order is correct."""
    b = Built(Case('n64-fp32', fork_min=True))
    plan = b.plan
    assert plan.wg_ws_main is not plan.wg_ws and S.conflicts(plan.bwd) == []
    again = b.rebuilt_backward()                                        # compiling again changes nothing by itself
    assert S.canonical(again) == S.canonical(plan.bwd)
    assert S.conflicts(again) == []
    plan.wg_ws_main = plan.wg_ws
    found = S.conflicts(b.rebuilt_backward())
    shared = [c for c in found if c.fork_symbol == c.main_symbol == 'hdy_conv_wgrad' and c.fork_arg == c.main_arg == 'workspace' and c.fork_write
              and c.main_write and c.fork_region.inside(plan.wg_ws)]
    assert shared and len(shared) == len(found), found[:5]
