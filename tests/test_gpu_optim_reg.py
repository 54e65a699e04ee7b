"""The fused Adam step, the density-L1 regulariser and the TV regulariser on the GPU, at the launch shapes training reaches,
held to the float64 references of tests/optim_reg_cases.py: tables of more than LRF_ADAM_MAX tensors, lrf_adam_step_pack with
more than ADAM_SMALL_CAP small tensors and with device scalars, unaligned and tail elements, lattices past one pass of
k_l1_fwd's grid-stride loop, TV tables up to LRF_TV_MAX.  Parameters, gradients and Adam state are views into buffers
filled with a sentinel pattern; the bytes outside the views are compared with the pattern after every step."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optim_reg_cases as K
from localrf_amd import FusedAdam
from localrf_amd import _native as N
from localrf_amd.field import _DensityL1Fn, _TVLossFn
from localrf_amd.optim import StaticAdamPlan
from util import PAD, Pool, make_field, make_rays, quiet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _kernel_constant(name, file="lrf_adam.inl"):
    """A `constexpr int` of the kernel sources, read from them: a changed constant moves the test's cases with it, or fails
    their assertions."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(N.__file__)), "csrc", file)).read()
    found = re.findall(r"constexpr int " + name + r" = (\d+);", src)
    assert len(found) == 1, name
    return int(found[0])


ADAM_SMALL_CAP = _kernel_constant("ADAM_SMALL_CAP")      # the small tensors k_adam_pack takes along


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().clone()


def _np64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _seeded(opt, p, m, v, step):
    """State at addresses of the test's choosing (state dicts interchange with torch.optim.Adam: these are its keys)."""
    opt.state[p] = {"step": step, "exp_avg": m, "exp_avg_sq": v}


def _within(got, ref, bound):
    return bool((np.abs(_np64(got).reshape(-1) - ref.reshape(-1)) <= bound.reshape(-1)).all())


# ------------------------------------------------------------------------------------------------------------ 2a
@pytest.mark.parametrize("n", K.ADAM_SIZES)
def test_adam_step_within_the_derived_bound(n):
    """lrf_adam_step, one tensor of n elements six times in one table: all four arrays 16-byte aligned (float4 path + scalar
    tail i + 4 > n), exactly one of p / g / m / v one float off (vec_ok false: scalar path throughout), and an aligned one
    with g = 0 and v = 0 (the denominator is eps).  Three steps with a changing lr; after EACH step every element of p, m, v
    lies within adam_step_ref's element-wise bound of the float64 step from the state the kernel started that step from,
    the gradients and every byte outside the views are untouched."""
    b1, b2 = K.ADAM_BETAS
    pools = [Pool(6 * (n + 2 * PAD + 4)) for _ in range(4)]
    variants = [None, 0, 1, 2, 3, "zero"]
    ps, opt_params = [], []
    for k, var in enumerate(variants):
        arrs = K.adam_arrays(n, 100 * n + k, zero_grad=(var == "zero"))
        views = [pool.take(a, mis=int(var == j)) for j, (pool, a) in enumerate(zip(pools, arrs))]
        p = torch.nn.Parameter(views[0])
        assert p.data_ptr() == views[0].data_ptr()
        p.grad = views[1]
        ps.append((p, views))
        opt_params.append(p)
    opt = FusedAdam(opt_params, lr=0.02, betas=K.ADAM_BETAS, eps=K.ADAM_EPS)
    for k, (p, views) in enumerate(ps):
        _seeded(opt, p, views[2], views[3], step=3 + k)
    for it in range(3):
        lr = opt.param_groups[0]["lr"]
        want = []
        for k, (p, (pv, gv, mv, vv)) in enumerate(ps):
            if it and variants[k] != "zero":                     # a new gradient, written in place: same address
                gv.copy_(torch.from_numpy(K.adam_arrays(n, 100 * n + k + 7 * it)[1]))
            step_size, bc2 = K.adam_scalars(lr, b1, b2, 3 + k + it + 1)
            want.append(K.adam_step_ref(_np64(pv), _np64(gv), _np64(mv), _np64(vv), step_size, bc2, b1, b2, K.ADAM_EPS))
        g_before = _bits(pools[1].buf)
        opt.step()
        torch.cuda.synchronize()
        for k, (p, (pv, gv, mv, vv)) in enumerate(ps):
            p1, m1, v1, E_p, E_m, E_v = want[k]
            assert _within(mv, m1, E_m), (n, variants[k], it, "m")
            assert _within(vv, v1, E_v), (n, variants[k], it, "v")
            assert _within(pv, p1, E_p), (n, variants[k], it, "p")
            assert int(opt.state[p]["step"]) == 3 + k + it + 1
        assert torch.equal(_bits(pools[1].buf), g_before)
        assert all(pool.intact() for pool in pools), (n, it)
        opt.param_groups[0]["lr"] = lr * 0.5


# ------------------------------------------------------------------------------------------------------- 2b, 2c
MAIN_SHAPES = [(1, 8, 9, 11), (1, 8, 13, 1), (1, 24, 9, 11), (1, 24, 13, 1), (27, 72), (128, 27), (128,), (3, 131), (5,), (4097,),
               (1, 8, 7, 5), (1, 8, 6, 1), (3, 128), (3,)]
POSE_SHAPES = [(3, 2), (3,), (1,)]
N_POSE = 150


class _Many:
    """A 14-tensor main optimiser (two groups) and 150 one-tensor optimisers, 164 tensors: three launches of at most
    LRF_ADAM_MAX.  Everything lives in sentinel pools; the state is pre-seeded with varied step counts."""

    def __init__(self, seed):
        r = np.random.default_rng(seed)
        shapes = MAIN_SHAPES + [POSE_SHAPES[i % 3] for i in range(N_POSE)]
        cap = sum(int(np.prod(s)) + 2 * PAD + 4 for s in shapes)
        self.pools = [Pool(cap) for _ in range(4)]
        self.params, self.steps = [], []
        for i, s in enumerate(shapes):
            p = torch.nn.Parameter(self.pools[0].take(r.standard_normal(s)))
            g = self.pools[1].take(np.zeros(s))
            m = self.pools[2].take(0.1 * r.standard_normal(s))
            v = self.pools[3].take(0.01 * r.standard_normal(s) ** 2)
            self.params.append((p, g, m, v))
            self.steps.append(i % 5)
        ps = [q[0] for q in self.params]
        self.main = FusedAdam([{"params": ps[:4], "lr": 0.02}, {"params": ps[4:14], "lr": 1e-3}], betas=K.ADAM_BETAS, eps=K.ADAM_EPS)
        self.pose = [FusedAdam([p], lr=(5e-3, 5e-4, 1e-3)[i % 3], betas=K.ADAM_BETAS, eps=K.ADAM_EPS) for i, p in enumerate(ps[14:])]
        self.opts = [self.main] * 14 + self.pose
        for opt, (p, g, m, v), st in zip(self.opts, self.params, self.steps):
            _seeded(opt, p, m, v, st)

    def lr(self, i):
        if i < 14:
            return self.main.param_groups[0 if i < 4 else 1]["lr"]
        return self.pose[i - 14].param_groups[0]["lr"]

    def decay(self, f):
        for o in [self.main] + self.pose:
            for grp in o.param_groups:
                grp["lr"] *= f

    def set_grads(self, it, seed, inactive, none_for_inactive):
        r = np.random.default_rng(seed + it)
        for i, (p, g, m, v) in enumerate(self.params):
            g.copy_(torch.from_numpy((r.standard_normal(g.shape) * 10.0 ** r.integers(-3, 2)).astype(np.float32)))
            p.grad = None if (none_for_inactive and i in inactive) else g

    def snapshot(self):
        return [(_bits(p), _bits(m), _bits(v)) for p, g, m, v in self.params]

    def step_counts(self):
        return [int(o.state[q[0]]["step"]) for o, q in zip(self.opts, self.params)]


def _inactive(it):
    """A different subset on each step: a third of the pose tensors, one tensor of each main group, across all three launches."""
    return {i for i in range(14, 14 + N_POSE) if i % 3 == it} | {1 + it, 6 + it}


def test_adam_step_many_over_more_than_one_table():
    """FusedAdam.step_many over 164 tensors (FusedAdam._launch splits them into launches of 64, 64 and 36): three steps, lr
    changed between them, another subset with .grad = None each time.  Stepped tensors within adam_step_ref's element-wise
    bound; untouched ones bit-identical in p, exp_avg and exp_avg_sq with their step count unchanged; nothing outside the
    views written."""
    b1, b2 = K.ADAM_BETAS
    M = _Many(seed=21)
    assert len(M.params) == 164 > 2 * N.LRF_ADAM_MAX
    for it in range(3):
        off = _inactive(it)
        M.set_grads(it, 50, off, none_for_inactive=True)
        before, counts = M.snapshot(), M.step_counts()
        want = {}
        for i, (p, g, m, v) in enumerate(M.params):
            if i not in off:
                step_size, bc2 = K.adam_scalars(M.lr(i), b1, b2, counts[i] + 1)
                want[i] = K.adam_step_ref(_np64(p), _np64(g), _np64(m), _np64(v), step_size, bc2, b1, b2, K.ADAM_EPS)
        FusedAdam.step_many([M.main] + M.pose)
        torch.cuda.synchronize()
        after, counts1 = M.snapshot(), M.step_counts()
        for i, (p, g, m, v) in enumerate(M.params):
            if i in off:
                assert all(torch.equal(a, b) for a, b in zip(before[i], after[i])), (it, i)
                assert counts1[i] == counts[i]
            else:
                p1, m1, v1, E_p, E_m, E_v = want[i]
                assert _within(m, m1, E_m) and _within(v, v1, E_v) and _within(p, p1, E_p), (it, i)
                assert counts1[i] == counts[i] + 1
                assert not torch.equal(before[i][0], after[i][0]), (it, i)
        assert all(pool.intact() for pool in M.pools), it
        M.decay(0.7)


def test_static_adam_plan_over_more_than_one_table():
    """The same 164 pairs as a StaticAdamPlan (lrf_adam_step_dev, each launch reading the device scalar table from its own
    first row: scalars_dev[part[0]:]), three eager launches with host_scalars(out, active=...) written before each: parameters
    and both state tensors bit-identical to a twin stepped through FusedAdam.step_many with .grad = None for the inactive
    tensors, inactive rows untouched, step counters equal."""
    A, B = _Many(seed=21), _Many(seed=21)
    plan = StaticAdamPlan(list(zip(B.opts, [q[0] for q in B.params])))
    assert len(plan) == 164
    host = torch.zeros(len(plan), 2, dtype=torch.float32).pin_memory()
    scalars_dev = torch.zeros(len(plan), 2, dtype=torch.float32, device=DEV)
    for it in range(3):
        off = _inactive(it)
        A.set_grads(it, 50, off, none_for_inactive=True)
        B.set_grads(it, 50, off, none_for_inactive=False)            # the plan bakes every gradient pointer in
        before = B.snapshot()
        FusedAdam.step_many([A.main] + A.pose)
        plan.host_scalars(host.numpy(), active={id(q[0]) for i, q in enumerate(B.params) if i not in off})
        for i in off:
            assert host[i, 0] == 0 and host[i, 1] == 0
        scalars_dev.copy_(host)
        plan.launch(scalars_dev)
        plan.bump_versions()
        torch.cuda.synchronize()
        a, b = A.snapshot(), B.snapshot()
        for i in range(164):
            assert all(torch.equal(x, y) for x, y in zip(a[i], b[i])), (it, i)
            if i in off:
                assert all(torch.equal(x, y) for x, y in zip(before[i], b[i])), (it, i)
        assert A.step_counts() == B.step_counts()
        assert all(pool.intact() for pool in B.pools), it
        A.decay(0.7)
        B.decay(0.7)


# ------------------------------------------------------------------------------------------------------------ 2d
def _pose_set(n_pose, seed):
    """n_pose one-tensor FusedAdam optimisers over sentinel pools -> (optimisers, [(p, g, m, v)], pools)."""
    r = np.random.default_rng(seed)
    shapes = [POSE_SHAPES[i % 3] for i in range(n_pose)]
    pools = [Pool(sum(int(np.prod(s)) + 2 * PAD + 4 for s in shapes) + PAD) for _ in range(4)]
    opts, params = [], []
    for i, s in enumerate(shapes):
        p = torch.nn.Parameter(pools[0].take(r.standard_normal(s)))
        g, m, v = pools[1].take(np.zeros(s)), pools[2].take(0.1 * r.standard_normal(s)), pools[3].take(0.01 * r.standard_normal(s) ** 2)
        o = FusedAdam([p], lr=(5e-3, 5e-4, 1e-3)[i % 3], betas=K.ADAM_BETAS, eps=K.ADAM_EPS)
        _seeded(o, p, m, v, i % 4)
        opts.append(o)
        params.append((p, g, m, v))
    return opts, params, pools


def _field_pair(grid):
    fa = quiet(make_field, list(grid), "cpu", seed=5).to(DEV)
    fb = quiet(make_field, list(grid), "cpu", seed=5).to(DEV)
    oa = FusedAdam(fa.get_optparam_groups(0.02, 1e-3), betas=K.ADAM_BETAS)
    ob = FusedAdam(fb.get_optparam_groups(0.02, 1e-3), betas=K.ADAM_BETAS, pack_field=fb)
    return fa, fb, oa, ob


def _field_count(opt):
    return sum(len(grp["params"]) for grp in opt.param_groups)


def _check_twins(fa, fb, oa, ob, pa, pb, tag):
    for (n, p), (_, q) in zip(fa.named_parameters(), fb.named_parameters()):
        assert torch.equal(_bits(p), _bits(q)), (tag, n)
        if p in oa.state:
            sa, sb = oa.state[p], ob.state[q]
            assert torch.equal(_bits(sa["exp_avg"]), _bits(sb["exp_avg"])) and torch.equal(_bits(sa["exp_avg_sq"]), _bits(sb["exp_avg_sq"])), (tag, n)
            assert int(sa["step"]) == int(sb["step"]), (tag, n)
    for i, (x, y) in enumerate(zip(pa, pb)):
        assert all(torch.equal(_bits(s), _bits(t)) for s, t in zip(x, y)), (tag, "pose", i)


def _check_cache(fb, built_lib, tag):
    """The cache the fused step left == a fresh pack of the stepped parameters (into a clone: the alignment gaps between the
    cache's sections are nobody's)."""
    cp, keep = fb._c_params()
    fresh = fb.layout.cache.clone()
    N.check(built_lib.lrf_pack_field(C.byref(cp), fresh.data_ptr(), torch.cuda.current_stream().cuda_stream), "lrf_pack_field")
    torch.cuda.synchronize()
    assert torch.equal(fresh.view(torch.int32), fb.layout.cache.view(torch.int32)), tag


PACK_GRIDS = [(24, 20, 28), (36, 33, 28)]            # non-cubic; 33: an odd plane width (one texel per thread, all channels)


@pytest.mark.parametrize("mode", ["step_many", "plan"])
@pytest.mark.parametrize("config", ["few", "many"])
@pytest.mark.parametrize("grid", PACK_GRIDS)
def test_adam_pack_with_pose_tensors(built_lib, grid, config, mode):
    """lrf_adam_step_pack with the per-frame tensors in its table.  few: the non-field tensors number <= ADAM_SMALL_CAP and
    k_adam_pack takes them along; many: more than ADAM_SMALL_CAP with the table still <= LRF_ADAM_MAX, they go through a second
    k_adam_multi launch whose row[] holds the caller's indices.  Through FusedAdam.step_many (host scalars) and through a
    StaticAdamPlan (device scalars; pose pairs in front of the field's so that rows and table positions differ; one field
    tensor and a few pose tensors inactive).  Every time: parameters and state bit-identical to a twin without pack_field
    stepped through step_many, the cache bit-identical to a fresh pack of the stepped parameters, the inactive field tensor
    packed but not stepped, nothing outside the pose views written."""
    fa, fb, oa, ob = _field_pair(grid)
    nf = _field_count(ob)
    n_pose = {"few": 30, "many": N.LRF_ADAM_MAX - nf}[config]
    small, table = nf - 12 + n_pose, nf + n_pose                       # twelve plane / line tensors are the pack kernel's own
    if config == "few":
        assert small <= ADAM_SMALL_CAP and table <= N.LRF_ADAM_MAX and n_pose > 12
    else:
        assert small > ADAM_SMALL_CAP and table <= N.LRF_ADAM_MAX
    posea, pa, pools_a = _pose_set(n_pose, 31)
    poseb, pb, pools_b = _pose_set(n_pose, 31)
    rays = make_rays(96, 3).to(DEV)
    fparams_b = [p for grp in ob.param_groups for p in grp["params"]]
    if mode == "plan":
        pairs = [(o, q[0]) for o, q in zip(poseb[:5], pb[:5])] + [(ob, p) for p in fparams_b] + [(o, q[0]) for o, q in zip(poseb[5:], pb[5:])]
        plan = StaticAdamPlan(pairs)
        host = torch.zeros(len(plan), 2, dtype=torch.float32).pin_memory()
        scalars_dev = torch.zeros(len(plan), 2, dtype=torch.float32, device=DEV)
    g = torch.Generator().manual_seed(9)
    for it in range(3):
        grads = {n: torch.randn(p.shape, generator=g).to(DEV) * 0.1 for n, p in fa.named_parameters()}
        pgrads = [torch.randn(q[0].shape, generator=g) * 0.1 for q in pa]
        off_field = "density_line.1" if (mode == "plan" or it == 1) else None
        off_pose = {2, 7, 7 + it, n_pose - 1} if mode == "plan" else {it}
        for f in (fa, fb):
            with torch.no_grad():
                f(rays, N_samples=64)                                   # builds / takes the cache
        for f, twin in ((fa, True), (fb, False)):
            for n, p in f.named_parameters():
                p.grad = None if (n == off_field and (twin or mode != "plan")) else grads[n].clone()
        for ps, twin in ((pa, True), (pb, False)):
            for i, (p, gv, m, v) in enumerate(ps):
                gv.copy_(pgrads[i])
                p.grad = None if (i in off_pose and (twin or mode != "plan")) else gv
        frozen = _bits(dict(fb.named_parameters())[off_field]) if off_field else None
        key_before = fb.layout.key
        FusedAdam.step_many([oa] + posea)
        if mode == "plan":
            assert plan.packs(fb)
            active = {id(p) for n, p in fb.named_parameters() if n != off_field} | {id(q[0]) for i, q in enumerate(pb) if i not in off_pose}
            plan.host_scalars(host.numpy(), active=active)
            scalars_dev.copy_(host)
            plan.launch(scalars_dev)
            plan.bump_versions()
        else:
            FusedAdam.step_many([ob] + poseb)
        torch.cuda.synchronize()
        assert fb.layout.key is not None and fb.layout.key != key_before and fb.layout.is_fresh(fb)
        _check_twins(fa, fb, oa, ob, pa, pb, (it,))
        _check_cache(fb, built_lib, it)
        if off_field:
            assert torch.equal(frozen, _bits(dict(fb.named_parameters())[off_field]))
        assert all(pool.intact() for pool in pools_b), it
        key = fb.layout.key
        with torch.no_grad():
            ra, _ = fa(rays, N_samples=64)
            rb, _ = fb(rays, N_samples=64)
        assert fb.layout.key == key                                     # the forward took the cache as the step left it
        assert torch.equal(ra, rb)


def test_adam_pack_is_off_over_the_table_limit(built_lib):
    """A table of LRF_ADAM_MAX + 1: the step runs as plain lrf_adam_step launches, the field's layout key is NOT marked
    fresh, the next forward repacks and renders what the twin renders; a plan over the same pairs does not claim to pack."""
    fa, fb, oa, ob = _field_pair(PACK_GRIDS[1])
    nf = _field_count(ob)
    n_pose = N.LRF_ADAM_MAX + 1 - nf
    posea, pa, _ = _pose_set(n_pose, 31)
    poseb, pb, pools_b = _pose_set(n_pose, 31)
    assert nf + n_pose == N.LRF_ADAM_MAX + 1
    rays = make_rays(96, 3).to(DEV)
    g = torch.Generator().manual_seed(9)
    for f in (fa, fb):
        with torch.no_grad():
            f(rays, N_samples=64)
    grads = {n: torch.randn(p.shape, generator=g).to(DEV) * 0.1 for n, p in fa.named_parameters()}
    for f in (fa, fb):
        for n, p in f.named_parameters():
            p.grad = grads[n].clone()
    for ps in (pa, pb):
        for p, gv, m, v in ps:
            gv.fill_(0.05)
            p.grad = gv
    plan = StaticAdamPlan([(ob, p) for grp in ob.param_groups for p in grp["params"]] + [(o, q[0]) for o, q in zip(poseb, pb)])
    assert not plan.packs(fb)
    key_before = fb.layout.key
    FusedAdam.step_many([oa] + posea)
    FusedAdam.step_many([ob] + poseb)
    torch.cuda.synchronize()
    assert fb.layout.key == key_before and not fb.layout.is_fresh(fb)
    _check_twins(fa, fb, oa, ob, pa, pb, "over")
    assert all(pool.intact() for pool in pools_b)
    with torch.no_grad():
        ra, _ = fa(rays, N_samples=64)
        rb, _ = fb(rays, N_samples=64)
    assert fb.layout.key != key_before and fb.layout.is_fresh(fb)      # repacked
    assert torch.equal(ra, rb)
    _check_cache(fb, built_lib, "over")


# ------------------------------------------------------------------------------------------------------------ 2e
def test_an_empty_parameter_is_left_alone(monkeypatch):
    """An empty parameter among others: FusedAdam.step, step_many and StaticAdamPlan leave it alone as torch.optim.Adam does
    (its state is created, its step advances), nothing of it reaches the native table (lrf_adam_step still refuses a null
    pointer), the other tensors are stepped exactly as without it."""
    tables = []
    real = N.launch

    def spy(name, dev, *args, **kw):
        if name.startswith("lrf_adam_step"):
            tab, count = args[0], args[1]
            assert len(tab) == count
            tables.append([(tab[i].p, tab[i].n) for i in range(count)])
        return real(name, dev, *args, **kw)
    monkeypatch.setattr(N, "launch", spy)

    def build(with_empty):
        r = np.random.default_rng(4)
        ps = [torch.nn.Parameter(torch.from_numpy(r.standard_normal(s).astype(np.float32)).to(DEV)) for s in ((5, 3), (7,), (4097,))]
        e = torch.nn.Parameter(torch.empty(0, 3, device=DEV))
        first = FusedAdam([ps[0]] + ([e] if with_empty else []) + [ps[1]], lr=0.01, betas=K.ADAM_BETAS)
        second = FusedAdam([ps[2]], lr=0.02, betas=K.ADAM_BETAS)
        return ps, e, first, second
    (pa, _, fa1, fa2), (pb, e, fb1, fb2) = build(False), build(True)
    cpu_e = torch.nn.Parameter(torch.empty(0, 3))
    cpu = torch.optim.Adam([cpu_e], lr=0.01, betas=K.ADAM_BETAS)
    assert e.numel() == 0
    plan_a = StaticAdamPlan([(fa1, pa[0]), (fa1, pa[1]), (fa2, pa[2])])
    plan_b = StaticAdamPlan([(fb1, pb[0]), (fb1, e), (fb1, pb[1]), (fb2, pb[2])])
    scal_a, scal_b = torch.zeros(3, 2, device=DEV), torch.zeros(4, 2, device=DEV)
    r = np.random.default_rng(8)
    for it, how in enumerate(["step", "step_many", "plan"]):
        for x, y in zip(pa, pb):
            x.grad = torch.from_numpy(r.standard_normal(tuple(x.shape)).astype(np.float32)).to(DEV)
            y.grad = x.grad.clone()
        e.grad = torch.empty(0, 3, device=DEV)
        cpu_e.grad = torch.empty(0, 3)
        cpu.step()
        tables.clear()
        if how == "step":
            fa1.step(); fa2.step(); n_a = len(tables); fb1.step(); fb2.step()
        elif how == "step_many":
            FusedAdam.step_many([fa1, fa2]); n_a = len(tables); FusedAdam.step_many([fb1, fb2])
        else:
            ha, hb = np.zeros((3, 2), np.float32), np.zeros((4, 2), np.float32)
            plan_a.host_scalars(ha); plan_b.host_scalars(hb)
            scal_a.copy_(torch.from_numpy(ha)); scal_b.copy_(torch.from_numpy(hb))
            plan_a.launch(scal_a); n_a = len(tables); plan_b.launch(scal_b)
            plan_a.bump_versions(); plan_b.bump_versions()
        torch.cuda.synchronize()
        assert sorted(n for t in tables[:n_a] for _, n in t) == sorted(n for t in tables[n_a:] for _, n in t) == [7, 15, 4097]
        assert all(p and n > 0 for t in tables for p, n in t), how
        for x, y in zip(pa, pb):
            assert torch.equal(_bits(x), _bits(y)), how
            sa, sb = (fa2 if x is pa[2] else fa1).state[x], (fb2 if y is pb[2] else fb1).state[y]
            assert torch.equal(_bits(sa["exp_avg"]), _bits(sb["exp_avg"])) and torch.equal(_bits(sa["exp_avg_sq"]), _bits(sb["exp_avg_sq"]))
            assert int(sa["step"]) == int(sb["step"]) == it + 1
        st = fb1.state[e]
        assert int(st["step"]) == int(cpu.state[cpu_e]["step"]) == it + 1
        assert st["exp_avg"].shape == st["exp_avg_sq"].shape == (0, 3) and e.shape == (0, 3)
    # the native entry point keeps refusing a null pointer
    tab = (N.LrfAdamTensor * 1)()
    tab[0].n = 0
    with pytest.raises(N.NativeError, match="null tensor pointer"):
        real("lrf_adam_step", torch.device(DEV), tab, 1, 0.9, 0.99, 1e-8)


# ------------------------------------------------------------------------------------------------------- 3: L1
class _Act:
    """What _DensityL1Fn reads of a field."""

    def __init__(self, relu):
        self.density_shift, self.fea2denseAct = K.L1_SHIFT, "relu" if relu else "softplus"


G_UP = 0.37


@functools.lru_cache(maxsize=None)
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@functools.lru_cache(maxsize=None)
def _l1_case(grid, relu):
    """Inputs, the float64 reference (computed once, shared, not modified) and the error of the float32 CPU evaluation of the
    reference expression against it, in the form the kernel is held to: (value relative, gradients per own absolute sum)."""
    planes, lines = K.l1_inputs(grid, relu, seed=11)
    val, grads, sums = K.density_l1_ref(planes, lines, K.L1_SHIFT, relu)
    v32, g32 = K.density_l1_torch(planes, lines, K.L1_SHIFT, relu, torch.float32, g_up=K.f32(G_UP))
    e_val = abs(v32 - val) / val
    e_grad = max(K.normalised_error(a, K.f32(G_UP) * b, K.f32(G_UP) * c) for a, b, c in zip(g32, grads, sums))
    return planes, lines, val, grads, sums, e_val, e_grad


@pytest.mark.parametrize("case", ["large-softplus"] + [f"{g[0]}x{g[1]}x{g[2]}-{'relu' if r else 'softplus'}" for g in K.L1_SMALL_GRIDS for r in (False, True)])
def test_density_l1_on_constructed_lattices(case):
    """lrf_density_l1_fwd/_bwd/_bwd_acc through _DensityL1Fn on raw tensors, against density_l1_ref.

    Lattices: one with 4096 CUs < n <= 1.3 x 4096 CUs (CUs read from the device: k_l1_fwd's capped grid-stride loop takes a
    second iteration; every plane above 4096 texels: l1_qchunk above its minimum of 8), (300, 20, 12) (a 300-long line:
    k_l1_bwd_line's stride of 256 comes round; a 240-texel plane), (33, 17, 9), (5, 3, 2) (planes smaller than a workgroup's
    four waves, a 2-long line).  Inputs: K.l1_inputs, banded away from the clamp (test_optim_reg_host.py checks the condition).

    Bounds, each from THIS case's float32 CPU evaluation of the reference expression, measured in the same form:
      value      |got - ref| / ref <= 4 x that error + u.  The u = 2^-24 is the representability floor: the value is returned
                 as one float32, which cannot be held closer than u to an arbitrary real, while a single evaluation's error
                 can come out below that by chance (1.0e-8 on the large lattice).  The CPU evaluation runs on one thread
                 (K.density_l1_torch), so the measured error is a property of the torch build, not of the core count.
      gradients  element-wise, relative to each element's own sum of absolute terms: 4 x that error, no floor.
      accumulate into pre-filled buffers: pre-fill + gradient under the gradient bound plus one rounding of the sum.

    Measured on an MI355X host with 256 CUs (float32-CPU error -> bound | kernel):
      case                  value                          gradients
      large softplus        1.0e-8 -> 1.0e-7 | 9.6e-8      2.8e-6 -> 1.1e-5 | 2.2e-7
      (300, 20, 12) softp.  1.1e-7 -> 4.9e-7 | 6.4e-8      1.6e-6 -> 6.6e-6 | 2.7e-7
      (300, 20, 12) relu    8.4e-8 -> 4.0e-7 | 1.0e-8      1.4e-6 -> 5.7e-6 | 2.2e-7
      (33, 17, 9) softplus  3.5e-8 -> 2.0e-7 | 3.5e-8      4.5e-7 -> 1.8e-6 | 1.7e-7
      (33, 17, 9) relu      7.0e-8 -> 3.4e-7 | 4.3e-9      6.7e-7 -> 2.7e-6 | 2.0e-7
      (5, 3, 2) softplus    6.2e-8 -> 3.1e-7 | 6.2e-8      1.9e-7 -> 7.4e-7 | 1.6e-7
      (5, 3, 2) relu        7.3e-8 -> 3.5e-7 | 1.0e-7      1.7e-7 -> 6.8e-7 | 1.9e-7"""
    if case == "large-softplus":
        grid, relu = K.l1_large_grid(_cus()), False
    else:
        gs, act = case.split("-")
        grid, relu = tuple(int(x) for x in gs.split("x")), act == "relu"
    planes, lines, val, grads, sums, e_val, e_grad = _l1_case(grid, relu)
    tol_val, tol_grad = 4 * e_val + K.U, 4 * e_grad
    print(f"[l1 {case}] float32-CPU error: value {e_val:.3e} gradient {e_grad:.3e}; bounds {tol_val:.3e} {tol_grad:.3e}")
    n = planes[0].shape[2] * planes[0].shape[3] * lines[0].shape[2]
    if case == "large-softplus":
        assert 4096 * _cus() < n <= 1.3 * 4096 * _cus()
        assert all(p.shape[2] * p.shape[3] > 4096 for p in planes)
        fractions, forbidden = K.l1_bands(planes, lines, K.L1_SHIFT, relu)      # the inputs' condition, at this device's grid
        assert forbidden == 0 and min(fractions) >= 0.10, (grid, fractions, forbidden)
    ts = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in planes + lines]
    g_up = torch.tensor(G_UP, device=DEV)
    out = _DensityL1Fn.apply(_Act(relu), *ts)
    (out * g_up).backward()
    got = float(out.detach())
    gu = K.f32(G_UP)
    errs = [K.normalised_error(_np64(t.grad), gu * g, gu * a) for t, g, a in zip(ts, grads, sums)]
    print(f"[l1 {case}] kernel: value {abs(got - val) / val:.3e} gradients {' '.join(f'{e:.2e}' for e in errs)}")
    assert abs(got - val) <= tol_val * val
    assert max(errs) <= tol_grad, errs
    # accumulate=True: added to what the buffers hold
    r = np.random.default_rng(5)
    fill = [(0.01 * r.standard_normal(a.shape)).astype(np.float32) for a in planes + lines]
    bufs = [torch.from_numpy(a).to(DEV) for a in fill]
    det = tuple(t.detach() for t in ts)
    out2, ws = _DensityL1Fn.run_forward(_Act(relu), det)
    _DensityL1Fn.run_backward(ws, det, g_up, bufs, accumulate=True)
    torch.cuda.synchronize()
    assert float(out2) == got
    for b, f, g, a in zip(bufs, fill, grads, sums):
        want = f.astype(np.float64) + gu * g
        assert (np.abs(_np64(b) - want) <= tol_grad * gu * a + K.U * np.abs(want) * (1 + tol_grad)).all()


# ------------------------------------------------------------------------------------------------------- 4: TV
TV_UP = 1.3
TV_K = 10


@functools.lru_cache(maxsize=None)
def _tv_case(name):
    xs = K.tv_inputs(K.TV_TABLES[name], seed=4)
    val, grads, sums = K.tv_ref(xs, K.TV_WEIGHT)
    v32, _ = K.tv_torch(xs, K.TV_WEIGHT, torch.float32, want_grads=False)
    return xs, val, grads, sums, (abs(v32 - val) / val if val else 0.0)


def _tv_run(xs):
    ts = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in xs]
    out = _TVLossFn.apply(K.TV_WEIGHT, *ts)
    (out * torch.tensor(TV_UP, device=DEV)).backward()
    torch.cuda.synchronize()
    return float(out.detach()), [_np64(t.grad) for t in ts]


def test_tv_single_element_is_exactly_zero():
    got, grads = _tv_run(_tv_case("single")[0])
    assert got == 0.0 and grads[0].shape == (1, 1, 1, 1) and grads[0].reshape(-1)[0] == 0.0


@pytest.mark.parametrize("name", ["blocks", "sixteen"])
def test_tv_tables_against_the_reference(name):
    """lrf_tv_loss_fwd/_bwd through _TVLossFn on raw [1,C,H,W] tensors, weight 0.7, upstream gradient 1.3, against tv_ref.
    blocks: an H = 1 and a W = 1 tensor, one of exactly three 4096-element blocks, blocks ending mid-row and mid-channel,
    differences across a block boundary along H and along W.  sixteen: a table of LRF_TV_MAX distinct shapes.

    Value: relative to tv_ref, 4 x the float32-CPU error of the reference module on this table.

    Gradients: element-wise |got - ref| <= gam(10) abs_sum_i.  10 = the roundings k_tv_bwd puts on a term
    coefficient x difference: the difference (1), the sum of the two differences of a direction (1), the coefficient
    ch / cw = 2 / (C (H-1) W) (2 products, 1 division), its product with the sum (1), the sum of the two directions (1),
    s = g_out weight 2 scale (2; the factor 2 is exact) and s times the bracket (1).

    Measured on an MI355X host: float32-CPU value errors 5.1e-8 (blocks) and 2.6e-8 (sixteen), bounds 2.0e-7 and 1.0e-7; the
    kernel returned the very float32 numbers the CPU did.  Kernel gradients: 3.5 u and 2.7 u of their absolute sums."""
    xs, val, grads, sums, _ = _tv_case(name)
    tol_val = 4 * _tv_case(name)[4]
    assert len(xs) == K.TV_MAX == 16 or name == "blocks"
    got, got_grads = _tv_run(xs)
    up = K.f32(TV_UP)
    errs = [K.normalised_error(a, up * b, up * c) / K.U for a, b, c in zip(got_grads, grads, sums)]
    print(f"[tv {name}] float32-CPU value error {_tv_case(name)[4]:.3e}, bound {tol_val:.3e}; kernel value {abs(got - val) / val:.3e}, "
          f"gradients {max(errs):.2f} u")
    assert abs(got - val) <= tol_val * val
    for a, b, c in zip(got_grads, grads, sums):
        assert (np.abs(a - up * b) <= K.gam(TV_K) * up * c).all()


def test_tv_refuses_seventeen_tensors_before_any_launch():
    """One tensor more than LRF_TV_MAX: NativeError, through autograd and at both entry points, and nothing is written."""
    xs = [torch.from_numpy(a).to(DEV) for a in K.tv_inputs([(1, 2, 3, 4)] * (K.TV_MAX + 1), seed=1)]
    with pytest.raises(N.NativeError):
        _TVLossFn.apply(K.TV_WEIGHT, *[x.clone().requires_grad_(True) for x in xs])
    pool = Pool(17 * (24 + 2 * PAD + 4) + 4096)
    grads = [pool.take(np.zeros((1, 2, 3, 4))) for _ in xs]
    ws, out = pool.take(np.zeros(1024)), pool.take(np.zeros(1))
    before = _bits(pool.buf)
    tab = _TVLossFn._table(xs, grads)
    assert N.lib().lrf_tv_workspace(tab, len(xs)) == 0
    with pytest.raises(N.NativeError):
        N.launch("lrf_tv_loss_fwd", torch.device(DEV), tab, len(xs), K.TV_WEIGHT, ws.data_ptr(), N.ptr(out))
    with pytest.raises(N.NativeError):
        N.launch("lrf_tv_loss_bwd", torch.device(DEV), tab, len(xs), K.TV_WEIGHT, N.ptr(out))
    torch.cuda.synchronize()
    assert torch.equal(_bits(pool.buf), before)
    got, _ = _tv_run([a.cpu().numpy() for a in xs[:K.TV_MAX]])           # sixteen of them are fine
    assert got > 0
