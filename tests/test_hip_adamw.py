"""dg_adamw_flat, dg_adamw_flat_devstep and optim.FlatAdamW against float64 over twelve steps (tests/adamw_cases.py: cases,
reference, floors and bars), and the two entries at their edges: lengths around the 4-wide and 256-wide boundaries with
guard elements behind n, the device counter, replay from a captured graph, zero gradients, lr = 0, non-finite gradients,
argument errors, pointers off 16-byte alignment.

Every test that holds a kernel to the bars prints the worst error / bar it measured (a result passes where this is <= 1)."""
import numpy as np
import pytest
import torch

import adamw_cases as ac

pytestmark = pytest.mark.gpu

ENTRIES = ("flat", "devstep")
GUARD = 64


def _L():
    from druggen_amd import _lib
    return _lib


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _sentinels(which, count):
    """NaNs with a payload that names the buffer and the slot: a guard that is read shows as well as one that is written."""
    bits = 0x7FC00000 + (which << 12) + np.arange(count, dtype=np.int64)
    return torch.from_numpy(bits.astype(np.int32)).view(torch.float32)


class _State:
    """p, g, m, v of n elements, each followed by GUARD sentinels, each ``offsets[k]`` floats into its allocation; the int32
    step counter.  ``p0`` / ``m0`` / ``v0``: float32 arrays (zeros by default)."""

    def __init__(self, n, p0=None, m0=None, v0=None, offsets=(0, 0, 0, 0), counter=0):
        self.n = n
        self.bufs = []
        for k, (off, init) in enumerate(zip(offsets, (p0, None, m0, v0))):
            whole = torch.empty(off + n + GUARD, dtype=torch.float32)
            whole[:off] = _sentinels(8 + k, off)
            whole[off:off + n] = torch.zeros(n) if init is None else torch.from_numpy(np.asarray(init, dtype=np.float32))
            whole[off + n:] = _sentinels(k, GUARD)
            whole = whole.cuda()
            assert whole.data_ptr() % 16 == 0
            self.bufs.append((whole, whole[off:]))
        self.p, self.g, self.m, self.v = (view for _, view in self.bufs)
        self.counter = torch.full((1,), counter, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return [t.data_ptr() for t in (self.p, self.g, self.m, self.v)]

    def set_grad(self, g):
        self.g[:self.n].copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)))

    def step(self, entry, h, t=None, n=None):
        n = self.n if n is None else n
        if entry == "flat":
            _L().launch("dg_adamw_flat", self.p, *self.ptrs(), n, *h, t)
        else:
            _L().launch("dg_adamw_flat_devstep", self.p, *self.ptrs(), n, *h, self.counter.data_ptr())

    def values(self):
        """p, m, v [n] as float64 numpy."""
        return tuple(t[:self.n].double().cpu().numpy() for t in (self.p, self.m, self.v))

    def guards_intact(self):
        for k, (whole, view) in enumerate(self.bufs):
            off = whole.numel() - view.numel()
            if not torch.equal(_bits(whole[:off]), _bits(_sentinels(8 + k, off))):
                return False
            if not torch.equal(_bits(view[self.n:]), _bits(_sentinels(k, GUARD))):
                return False
        return True


def _hold(entry, c, offsets=(0, 0, 0, 0)):
    """Run case c through ``entry`` step by step against the bars; -> the final state.  Asserts guards, the untouched
    gradient and (devstep) the counter after every step."""
    st = _State(c.n, c.p0, offsets=offsets)
    bad, worst = [], {}
    for t in range(1, c.steps + 1):
        st.set_grad(c.grads[t - 1])
        before = _bits(st.g[:c.n])
        st.step(entry, c.h, t)
        p, m, v = st.values()
        bad += ac.failures(c, t, p, m, v, label=entry, worst_so_far=worst)
        assert torch.equal(_bits(st.g[:c.n]), before), f"{entry} {c.name} step {t}: the gradient was written"
        assert st.guards_intact(), f"{entry} {c.name} step {t}: an element outside [0, n) was written"
        if entry == "devstep":
            assert int(st.counter) == t
    print(f"[{entry}] {c.name}: worst error / bar: " + "  ".join(f"{k} {w:.3g}" for k, w in worst.items()))
    assert not bad, "\n".join(bad)
    return st


# ------------------------------------------------------------------------------------------------ both entries against float64
@pytest.mark.parametrize("init", ac.INITS)
@pytest.mark.parametrize("hyper", range(len(ac.HYPERS)))
@pytest.mark.parametrize("entry", ENTRIES)
def test_entry_meets_the_bars_at_every_one_of_twelve_steps(entry, hyper, init):
    """dg_adamw_flat(step=t) and dg_adamw_flat_devstep (counter from 0), 4099 elements, every hyper-parameter set, both
    initialisations.  With the bias corrections of the device-step kernel evaluated in float32 (1.0f - powf(beta2, t)) the
    zero-initialised cases of sets 1 to 4 miss the bar by 1.7 to 26 (tests/test_adamw_cases_host.py)."""
    _hold(entry, ac.case(hyper, init))


@pytest.mark.parametrize("n", ac.LENGTHS)
@pytest.mark.parametrize("entry", ENTRIES)
def test_lengths_around_the_vector_and_block_boundaries_and_guards(entry, n):
    """n around 4 (float4 body / scalar tail), 256 and 1024 (blocks of either kernel): the first n elements meet the bars,
    the gradient and the 64 sentinels behind each of the four buffers keep their bits."""
    for init in ac.INITS:
        _hold(entry, ac.case(0, init).prefix(n, ac.SHORT_STEPS))


# ------------------------------------------------------------------------------------------------ the device counter
def _shared_state():
    """A nonzero (p, m, v, g): the spread case of set 1 after five steps, and the sixth gradient."""
    c = ac.case(0, "spread")
    f = lambda k: c.ref[k][4].astype(np.float32)
    return c, f("p"), f("m"), f("v"), c.grads[5]


@pytest.mark.parametrize("t", [1, 2, 7, 1000, 100000])
def test_devstep_with_a_preset_counter_agrees_with_the_host_step(t):
    """Counter preset to t - 1: the call increments it, THEN uses it -- the same update as dg_adamw_flat(step=t) within
    4 floor lr + 2^-23 |p| per element (not bit for bit: host and device pow may differ in the last double bit)."""
    c, p, m, v, g = _shared_state()
    dev, host = _State(c.n, p, m, v, counter=t - 1), _State(c.n, p, m, v)
    for st in (dev, host):
        st.set_grad(g)
    dev.step("devstep", c.h)
    host.step("flat", c.h, t)
    assert int(dev.counter) == t and int(host.counter) == 0
    (pd, md, vd), (ph, mh, vh) = dev.values(), host.values()
    # the moments do not depend on the step count (two kernels: a rounding of each term is allowed for, no more)
    assert np.all(np.abs(md - mh) <= 2.0 ** -22 * (np.abs(m) + np.abs(g))) and np.all(np.abs(vd - vh) <= 2.0 ** -22 * vh)
    diff = np.abs(pd - ph)
    ulps = diff / np.spacing(np.abs(ph).astype(np.float32)).astype(np.float64)
    print(f"t = {t}: largest |devstep - host| = {diff.max():.3g} ({ulps.max():.3g} ulp)")
    assert np.all(diff <= 4 * c.floor * c.h[0] + 2.0 ** -23 * np.abs(ph))
    assert float(np.abs(ph - p.astype(np.float64)).max()) > 0
    assert dev.guards_intact() and host.guards_intact()


def test_graph_replay_is_bit_identical_to_eager_calls():
    """One captured devstep launch (counter bump -> update: a single chain), replayed six times with a new gradient copied
    into the static buffer before each replay: parameters and moments bit-identical to six eager calls, counter 6."""
    n, steps = 1027, 6
    c = ac.case(0, "spread").prefix(n, steps)
    eager = _State(n, c.p0)
    for t in range(steps):
        eager.set_grad(c.grads[t])
        eager.step("devstep", c.h)
    static = _State(n, c.p0)
    start = [t.clone() for t in (static.p, static.m, static.v)]
    static.set_grad(c.grads[0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        static.step("devstep", c.h)                      # warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static.step("devstep", c.h)
    for dst, src in zip((static.p, static.m, static.v), start):      # back to the start: the warm-up was a real step
        dst.copy_(src)
    static.counter.zero_()
    for t in range(steps):
        static.set_grad(c.grads[t])
        graph.replay()
    torch.cuda.synchronize()
    assert int(static.counter) == steps and int(eager.counter) == steps
    for name, a, b in zip("pmv", (static.p, static.m, static.v), (eager.p, eager.m, eager.v)):
        assert torch.equal(_bits(a), _bits(b)), name
    bad = ac.failures(c, steps, *static.values(), label="replay")
    assert not bad, "\n".join(bad)
    assert static.guards_intact()


# ------------------------------------------------------------------------------------------------ values
def _f32(x):
    return torch.from_numpy(np.asarray(x, dtype=np.float32))


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_gradient_is_pure_decay(entry):
    """g == 0: p becomes exactly p * (1.0f - lr*wd), m and v stay 0.  The kernels form the factor with one rounding
    (fmaf(-lr, wd, 1)); for every hyper-parameter set here that is also what the C expression gives with the product rounded
    first, so the statement does not depend on how a compiler contracts it."""
    from fractions import Fraction
    for h in ac.HYPERS:
        lr, wd = np.float32(h[0]), np.float32(h[4])
        once = np.float32(float(1 - Fraction(float(lr)) * Fraction(float(wd))))      # (exact in double before the last rounding)
        assert once == np.float32(1) - lr * wd, h
    c = ac.case(4, "spread").prefix(1027, 3)                                # weight_decay = .1
    lr, wd = np.float32(c.h[0]), np.float32(c.h[4])
    decay = np.float32(1) - lr * wd
    assert decay.dtype == np.float32 and decay < 1
    st, want = _State(c.n, c.p0), c.p0.copy()
    for t in range(1, 4):
        st.step(entry, c.h, t)
        want = want * decay
        assert want.dtype == np.float32
        assert torch.equal(_bits(st.p[:c.n]), _bits(_f32(want))), t
        assert not st.m[:c.n].any() and not st.v[:c.n].any()
    assert st.guards_intact()


@pytest.mark.parametrize("entry", ENTRIES)
def test_zero_learning_rate_leaves_the_parameters_and_moves_the_moments(entry):
    src = ac.case(0, "spread").prefix(1027, 3)
    h = (0.0,) + src.h[1:]
    c = ac.Case("lr = 0", h, "spread", src.p0, src.grads, ac.reference(src.p0, src.grads, h), src.floor)
    st = _State(c.n, c.p0)
    start = _bits(st.p[:c.n])
    for t in range(1, 4):
        st.set_grad(c.grads[t - 1])
        st.step(entry, c.h, t)
        assert torch.equal(_bits(st.p[:c.n]), start), t
        p, m, v = st.values()
        rm, rv = ac.moment_ratios(c, t, m, v)
        assert float(rm.max()) <= 1 and float(rv.max()) <= 1 and m.any() and v.all()


@pytest.mark.parametrize("entry", ENTRIES)
def test_non_finite_gradients_stay_in_their_elements_and_spread_as_in_torch(entry):
    """+inf, -inf and NaN at positions 1, 6 and n - 1 of the second step's gradient (n = 1027: inside the first and the
    second float4, and in the scalar tail): the non-finite pattern of p, m, v is torch.optim.AdamW's on the same float32
    GPU tensors, and every other element -- the neighbours inside the same float4 too -- has the bits of a run without them."""
    c = ac.case(0, "spread").prefix(1027, 2)
    n = c.n
    planted = c.grads[1].copy()
    where = {1: np.inf, 6: -np.inf, n - 1: np.nan}
    for i, x in where.items():
        planted[i] = x
    clean, dirty = _State(n, c.p0), _State(n, c.p0)
    ref = torch.nn.Parameter(_f32(c.p0).cuda())
    lr, b1, b2, eps, wd = c.h
    opt = torch.optim.AdamW([ref], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    for t, (g_clean, g_dirty) in enumerate(((c.grads[0], c.grads[0]), (c.grads[1], planted)), start=1):
        clean.set_grad(g_clean)
        dirty.set_grad(g_dirty)
        clean.step(entry, c.h, t)
        dirty.step(entry, c.h, t)
        ref.grad = _f32(g_dirty).cuda()
        opt.step()
    state = opt.state[ref]
    others = torch.ones(n, dtype=torch.bool)
    others[list(where)] = False
    pattern = lambda x: torch.stack([torch.isnan(x), torch.isposinf(x), torch.isneginf(x)]).cpu()
    for name, mine, theirs, base in (("p", dirty.p, ref.detach(), clean.p), ("m", dirty.m, state["exp_avg"], clean.m),
                                     ("v", dirty.v, state["exp_avg_sq"], clean.v)):
        assert torch.equal(pattern(mine[:n]), pattern(theirs)), name
        assert not torch.isfinite(mine[:n].cpu()[~others]).any(), name
        assert torch.equal(_bits(mine[:n])[others], _bits(base[:n])[others]), name
    assert dirty.guards_intact()


# ------------------------------------------------------------------------------------------------ arguments
def _raw_call(entry, st, n, h, last):
    lib = _L().load()
    fn = lib.dg_adamw_flat if entry == "flat" else lib.dg_adamw_flat_devstep
    def call(ptrs=None, n=n, last=last):
        return fn(*(st.ptrs() if ptrs is None else ptrs), n, *h, last, _L().stream_of(st.p))
    return lib, call


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_and_the_empty_call(entry):
    """A null pointer, n < 0 and step < 1 give a nonzero status and a message; n == 0 returns 0 and touches nothing (the
    counter included).  Nothing is launched by any of these calls."""
    c = ac.case(0, "spread").prefix(8, 1)
    st = _State(c.n, c.p0, counter=3)
    st.set_grad(c.grads[0])
    torch.cuda.synchronize()
    before = [_bits(whole) for whole, _ in st.bufs]
    h = c.h
    lib, call = _raw_call(entry, st, c.n, h, 1 if entry == "flat" else st.counter.data_ptr())

    def refused(status):
        msg = lib.dg_last_error_string()
        return status != 0 and bool(msg) and ("dg_adamw_flat" in msg.decode())

    for k in range(4):
        ptrs = st.ptrs()
        ptrs[k] = None
        assert refused(call(ptrs=ptrs)), k
    assert refused(call(n=-1))
    if entry == "flat":
        assert refused(call(last=0)) and refused(call(last=-5))
    else:
        assert refused(call(last=None))
    assert call(n=0) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(whole), b) for (whole, _), b in zip(st.bufs, before))
    assert int(st.counter) == 3
    assert call() == 0                                  # and the same call with n elements goes through
    torch.cuda.synchronize()
    assert int(st.counter) == (3 if entry == "flat" else 4)
    assert not torch.equal(_bits(st.p[:c.n]), before[0][:c.n]) and st.guards_intact()


# ------------------------------------------------------------------------------------------------ alignment of dg_adamw_flat
def test_flat_with_pointers_off_16_byte_alignment_is_bit_identical():
    """Each of the four pointers 1, 2 and 3 floats into its allocation, one at a time and all four together: dg_adamw_flat
    takes its scalar body (no access wider than a float) and gives the bits of the aligned run, guards on both sides intact."""
    c = ac.case(0, "spread").prefix(1027, 3)
    aligned = _hold("flat", c)
    want = [_bits(t[:c.n]) for t in (aligned.p, aligned.m, aligned.v)]
    layouts = [tuple(off if k == j else 0 for k in range(4)) for j in range(4) for off in (1, 2, 3)]
    layouts += [(off,) * 4 for off in (1, 2, 3)] + [(1, 2, 3, 0)]
    for offsets in layouts:
        st = _hold("flat", c, offsets=offsets)
        assert any(ptr % 16 for ptr in st.ptrs())
        for name, t, w in zip("pmv", (st.p, st.m, st.v), want):
            assert torch.equal(_bits(t[:c.n]), w), (offsets, name)


# ------------------------------------------------------------------------------------------------ FlatAdamW
SHAPES = [(64, 128), (128,), (384,), (5,), (7, 3), (16, 384)]      # (128,) and (384,) start at zero: a bias, a LayerNorm beta
ZERO = (1, 2)


def _flat_adamw_case(hyper):
    sizes = [int(np.prod(s)) for s in SHAPES]
    total = sum(sizes)
    h = ac.widened(ac.HYPERS[hyper])
    grads = ac.gradients(total, 100 + hyper)
    p0 = ac.initial(total, "spread", 100 + hyper)
    rows = np.zeros(total, dtype=bool)
    bounds = np.cumsum([0] + sizes)
    for k in ZERO:
        p0[bounds[k]:bounds[k + 1]] = 0
        rows[bounds[k]:bounds[k + 1]] = True
    c = ac.Case(f"FlatAdamW set {hyper + 1}", h, "spread", p0, grads, ac.reference(p0, grads, h), ac.floor_of(grads, h))
    assert c.floor < ac.FLOOR_MAX
    return c, rows, bounds


def _parameters(c, bounds):
    return [torch.nn.Parameter(_f32(c.p0[bounds[k]:bounds[k + 1]]).reshape(s).cuda()) for k, s in enumerate(SHAPES)]


def _give(ps, c, bounds, t):
    for k, p in enumerate(ps):
        p.grad = _f32(c.grads[t - 1][bounds[k]:bounds[k + 1]]).reshape(p.shape).cuda()


@pytest.mark.parametrize("hyper", [1, 3])
def test_flat_adamw_twelve_steps_against_float64_torch(hyper):
    """optim.FlatAdamW over mixed shapes, two of them zero-initialised vectors, and one parameter that never gets a gradient:
    every parameter inside its bar (zero / spread) against float64 torch.optim.AdamW at every step, the device counter equal
    to step_count, the dead parameter untouched."""
    from druggen_amd.optim import FlatAdamW
    c, rows, bounds = _flat_adamw_case(hyper)
    t64 = ac.torch_adamw(c.p0, c.grads, c.h, torch.float64)
    assert all(np.abs(t64[k] - c.ref[k]).max() <= 2.0 ** -48 * np.abs(c.ref[k]).max() for k in "pmv")
    ps = _parameters(c, bounds)
    dead = torch.nn.Parameter(torch.randn(9, generator=torch.Generator().manual_seed(0)).cuda())
    dead0 = dead.detach().clone()
    lr, b1, b2, eps, wd = c.h
    opt = FlatAdamW(ps[:3] + [dead] + ps[3:], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    bad, worst = [], {}
    for t in range(1, ac.T + 1):
        _give(ps, c, bounds, t)
        opt.step()
        assert int(opt.device_step) == opt.step_count == t
        got = torch.cat([p.detach().reshape(-1) for p in ps]).double().cpu().numpy()
        bad += ac.failures(c, t, got, opt.exp_avg.double().cpu().numpy(), opt.exp_avg_sq.double().cpu().numpy(),
                           label="FlatAdamW", rows=rows, worst_so_far=worst)
        opt.zero_grad()
    print(f"{c.name}: floor {c.floor:.3g}  worst error / bar: " + "  ".join(f"{k} {w:.3g}" for k, w in worst.items()))
    assert not bad, "\n".join(bad)
    assert torch.equal(dead, dead0) and dead.grad is None
    assert all(p.data_ptr() >= opt.flat_param.data_ptr() for p in ps)


def test_a_late_first_gradient_under_one_global_step_count_is_not_torch():
    """Why FlatAdamW refuses a change of the live set: one step count serves the whole buffer, so an element with fresh (zero)
    moments that is first stepped at t = 3 moves by lr r sign(g), r = (1 - b1) / (1 - b1^3) / sqrt((1 - b2) / (1 - b2^3))
    = 0.639, where torch.optim.AdamW -- one step count per parameter -- moves it by lr sign(g)."""
    c = ac.case(3, "zero").prefix(257, 1)                     # weight_decay = 0
    lr, b1, b2, eps, wd = c.h
    st = _State(c.n, c.p0)
    st.set_grad(c.grads[0])
    st.step("flat", c.h, 3)
    g = c.grads[0].astype(np.float64)
    big = np.abs(g) > 1e4 * eps
    r = (1 - b1) / (1 - b1 ** 3) / np.sqrt((1 - b2) / (1 - b2 ** 3))
    assert 0.63 < r < 0.65 and big.sum() > 100
    p = st.values()[0]
    assert np.allclose(p[big], -lr * r * np.sign(g[big]), rtol=1e-3, atol=0)
    assert np.allclose(c.ref["p"][0][big], -lr * np.sign(g[big]), rtol=1e-3, atol=0)      # torch's (and step=1's) first step


def test_flat_adamw_refuses_a_change_of_the_live_set():
    """A parameter that gets its first gradient at step 3, and one that stops getting one: RuntimeError naming them, nothing
    stepped."""
    from druggen_amd.optim import FlatAdamW
    c, rows, bounds = _flat_adamw_case(1)
    ps = _parameters(c, bounds)
    late = torch.nn.Parameter(torch.ones(9).cuda())
    opt = FlatAdamW(ps[:3] + [late] + ps[3:], lr=c.h[0])
    for t in (1, 2):
        _give(ps, c, bounds, t)
        opt.step()
        opt.zero_grad()
    before = opt.flat_param.clone()
    _give(ps, c, bounds, 3)
    late.grad = torch.ones(9).cuda()
    with pytest.raises(RuntimeError, match=r"joined: #3 \(9,\); left: none"):
        opt.step()
    opt.zero_grad()
    _give(ps, c, bounds, 3)
    ps[1].grad = None
    ps[4].grad = None
    with pytest.raises(RuntimeError, match=r"joined: none; left: #1 \(128,\), #5 \(7, 3\)"):
        opt.step()
    assert opt.step_count == 2 and int(opt.device_step) == 2 and torch.equal(opt.flat_param, before)
    assert torch.equal(late.detach().cpu(), torch.ones(9))
    ps[1].grad = _f32(c.grads[2][bounds[1]:bounds[2]]).cuda()      # the original set again: the optimizer goes on
    ps[4].grad = _f32(c.grads[2][bounds[4]:bounds[5]]).reshape(7, 3).cuda()
    opt.step()
    assert opt.step_count == 3 and int(opt.device_step) == 3 and not torch.equal(opt.flat_param, before)
