"""The dense side of the heads, called by name: ``ops.linear_grouped`` (linear.hip: ``ocn_linear_grouped``, one to five Linear
layers of one (K, N) per launch), ``ops.linear_t`` (the input gradient), ``ops.fill_rows`` and the panel cache, plus the fused
heads at the widths / LayerNorm settings no accuracy test reaches.

Reference: an fp64 evaluation of the documented epilogue order (ocn_hip.h): + bias -> LayerNorm -> ReLU -> * scale ->
(dot | store + addend).  Two bars, both the project's own:
  * outputs that are a GEMM and exactly-rounded elementwise steps: the bar of ``test_linear_bf16x6`` — the error against fp64
    is at most max(2 x the error of torch's fp32 evaluation, 2e-7 x max |exact|);
  * outputs after a LayerNorm or the trailing dot: atol = rtol = 1e-5 against fp64 (BASELINE.json north star).
What is exact in IEEE fp32 (one more multiply, one more add, a row that moved, a group that moved) is asserted on bits.
Every output buffer starts as a sentinel NaN pattern and has guard rows behind it; what the launch must not touch is compared
as int32."""
import copy
import itertools
from functools import partial

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENT = 0x7FC0BEEF                      # a quiet NaN that no computation here produces
GUARD = 2                              # sentinel rows behind every output
EPS = 1e-5
RANGE_M = 300
RANGES = [(0, 0), (0, 300), (5, 131), (128, 129), (299, 300), (-3, 40), (250, 1000), (200, 100), (300, 300)]


def sent(rows, cols):
    return torch.full((rows, cols), SENT, dtype=torch.int32, device=DEV).view(torch.float32)


def is_sent(t):
    return bool((t.view(torch.int32) == SENT).all())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def clamp(rng, M):
    lo, hi = max(rng[0], 0), min(rng[1], M)
    return (lo, hi) if hi > lo else (0, 0)


def dev_range(rng):
    return torch.tensor(rng, dtype=torch.int64, device=DEV)


def make_x(M, K, seed):
    """Rows and columns of mixed magnitude (as the wgrad tests build theirs): a mix-up of rows or of k positions shows."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g) * torch.logspace(-2, 0.5, K) * (0.25 + 3.0 * torch.rand(M, 1, generator=g))
    return x.to(DEV)


class Layer:
    """One Linear [N, K] with everything its epilogue can take."""

    def __init__(self, K, N, seed):
        g = torch.Generator().manual_seed(1000 + seed)
        self.K, self.N = K, N
        self.W = (torch.randn(N, K, generator=g) / K ** 0.5 * (0.5 + torch.rand(N, 1, generator=g))).to(DEV)
        self.b = torch.randn(N, generator=g).to(DEV)
        self.gamma = (1.0 + 0.5 * torch.randn(N, generator=g)).to(DEV)
        self.beta = torch.randn(N, generator=g).to(DEV)                      # negative entries: ReLU after LayerNorm bites
        self.dotw = (torch.randn(1, N, generator=g) / N ** 0.5).to(DEV)
        self.dotb = torch.randn(1, generator=g).to(DEV)


def scalar(v):
    return None if v is None else torch.tensor([v], dtype=torch.float32, device=DEV)


def full_addend(M, N, seed):
    """[M, N] inside a wider buffer (row stride N + 8, starting 4 floats in), with guard rows behind it."""
    g = torch.Generator().manual_seed(2000 + seed)
    return torch.randn(M + GUARD, N + 8, generator=g).to(DEV)[:M, 4:4 + N]


def row_addend(N, seed):
    g = torch.Generator().manual_seed(3000 + seed)
    return torch.randn(1, N, generator=g).to(DEV)


def evaluate(x, L, ep, dt):
    """The documented epilogue order in precision ``dt``."""
    y = F.linear(x.to(dt), L.W.to(dt), L.b.to(dt) if ep.get("bias") else None)
    if ep.get("ln"):
        y = F.layer_norm(y, (L.N,), L.gamma.to(dt), L.beta.to(dt), EPS)
    if ep.get("relu"):
        y = torch.relu(y)
    if ep.get("scale") is not None:
        y = y * ep["scale"].to(dt)
    if ep.get("dot"):
        return y @ L.dotw.to(dt).t() + L.dotb.to(dt)
    if ep.get("addend") is not None:
        y = y + ep["addend"].to(dt)
    return y


def group(x, L, y, ep, **extra):
    g = dict(x=x, weight=L.W, y=y, bias=L.b if ep.get("bias") else None,
             ln=(L.gamma, L.beta, EPS) if ep.get("ln") else None, relu=bool(ep.get("relu")), scale=ep.get("scale"),
             addend=ep.get("addend"), add_bcast=bool(ep.get("bcast")), dot=(L.dotw, L.dotb) if ep.get("dot") else None)
    g.update(extra)
    return g


def launch(x, L, ep, **extra):
    """One group into a sentinel buffer; its guard rows are checked here.  Returns the [M, N] (or [M, 1]) rows."""
    from ocn_amd import ops
    M = x.shape[0]
    buf = sent(M + GUARD, 1 if ep.get("dot") else L.N)
    ops.linear_grouped([group(x, L, buf[:M], ep, **extra)], L.K, L.N)
    assert is_sent(buf[M:]), "a row behind the last one was written"
    return buf[:M]


def check(got, x, L, ep):
    """The bar that applies to this epilogue (module docstring)."""
    exact = evaluate(x, L, ep, torch.float64)
    assert got.shape == exact.shape and bool(torch.isfinite(got).all()), ep
    err = (got.double() - exact).abs().max().item()
    if ep.get("ln") or ep.get("dot"):
        assert torch.allclose(got.double(), exact, atol=1e-5, rtol=1e-5), (err, tuple(x.shape), L.N, ep)
    else:
        err32 = (evaluate(x, L, ep, torch.float32).double() - exact).abs().max().item()
        assert err <= max(2.0 * err32, 2e-7 * exact.abs().max().item()), (err, err32, tuple(x.shape), L.N, ep)


# ---- 1. the epilogue against fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bias,ln,relu", list(itertools.product((False, True), repeat=3)))
def test_epilogue_matrix_against_fp64(hiplib, bias, ln, relu):
    M, K, N = 129, 80, 64
    L, x = Layer(K, N, 1), make_x(M, K, 1)
    for scale in (None, 0.6, -1.7):
        for tail in ("store", "addend", "bcast", "dot"):
            ep = dict(bias=bias, ln=ln, relu=relu, scale=scalar(scale), dot=tail == "dot")
            if tail == "addend":
                ep["addend"] = full_addend(M, N, 1)
            elif tail == "bcast":
                ep.update(addend=row_addend(N, 1), bcast=True)
            check(launch(x, L, ep), x, L, ep)


# every N with two K (the mix layer's K = 2N among them), every K with one N at least; then every M at one (K, N)
SHAPES = [(129, 16, 32), (129, 64, 32), (129, 48, 64), (129, 80, 64), (129, 64, 128), (129, 16, 128), (129, 80, 256), (257, 512, 256)]
SHAPES += [(M, 80, 128) for M in (1, 31, 32, 33, 127, 128, 257)]


@pytest.mark.parametrize("M,K,N", SHAPES, ids=lambda v: str(v))
def test_shapes_against_fp64(hiplib, M, K, N):
    L, x = Layer(K, N, M + K + N), make_x(M, K, M + K + N)
    for ep in (dict(bias=True),
               dict(bias=True, relu=True, scale=scalar(-1.7), addend=full_addend(M, N, 2)),
               dict(bias=True, ln=True, relu=True, dot=True),
               dict(ln=True, scale=scalar(0.6), addend=row_addend(N, 2), bcast=True)):
        check(launch(x, L, ep), x, L, ep)


# ---- 2. relations that are exact in fp32 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [False, True])
@pytest.mark.parametrize("M,K,N", [(257, 80, 128), (129, 48, 32)])
def test_scale_addend_and_relu_are_single_exact_steps(hiplib, M, K, N, ln):
    L, x = Layer(K, N, 3), make_x(M, K, 3)
    base = dict(bias=True, ln=ln)
    raw = launch(x, L, base)
    act = launch(x, L, dict(base, relu=True))
    assert bool((raw < 0).any()) and torch.equal(act, torch.relu(raw))
    add, row = full_addend(M, N, 3), row_addend(N, 3)
    assert torch.equal(launch(x, L, dict(base, relu=True, addend=add)), act + add)
    assert torch.equal(launch(x, L, dict(base, relu=True, addend=row, bcast=True)), act + row)
    for s in (0.6, -1.7):
        sc = scalar(s)
        scaled = launch(x, L, dict(base, relu=True, scale=sc))
        assert torch.equal(scaled, act * sc), s                             # after ReLU: a negative scale flips the sign of what survived
        assert s > 0 or (bool((scaled <= 0).all()) and bool((scaled < 0).any()))
        assert torch.equal(launch(x, L, dict(base, relu=True, scale=sc, addend=add)), act * sc + add), s
        assert torch.equal(launch(x, L, dict(base, relu=True, scale=sc, addend=row, bcast=True)), act * sc + row), s
        assert torch.equal(launch(x, L, dict(base, scale=sc)), raw * sc), s


# ---- 3. strides ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,K,N", [(129, 48, 64), (257, 80, 256)])
def test_strided_x_and_y_halves(hiplib, M, K, N):
    from ocn_amd import ops
    L, x = Layer(K, N, 4), make_x(M, K, 4)
    ep = dict(bias=True, relu=True, scale=scalar(0.6), addend=full_addend(M, N, 4))
    want = launch(x, L, ep)
    wide_x = sent(M + GUARD, K + 8)                                         # what lies around X is NaN: reading it would show
    wide_x[:M, 4:4 + K] = x
    xs = wide_x[:M, 4:4 + K]
    assert same_bits(launch(xs, L, ep), want)
    for half in (0, 1):
        buf = sent(M + GUARD, 2 * N)
        ops.linear_grouped([group(xs, L, buf[:M, half * N:(half + 1) * N], ep)], K, N)
        assert same_bits(buf[:M, half * N:(half + 1) * N], want), half
        assert is_sent(buf[:M, (1 - half) * N:(2 - half) * N]) and is_sent(buf[M:]), half
    buf = sent(M + GUARD, N + 4)                                            # pad columns behind each row
    ops.linear_grouped([group(x, L, buf[:M, :N], ep)], K, N)
    assert same_bits(buf[:M, :N], want) and is_sent(buf[:, N:]) and is_sent(buf[M:])


# ---- 4. a group's result does not depend on the groups around it -------------------------------------------------------------------
def test_group_position_independence(hiplib):
    from ocn_amd import ops
    K, N, M = 80, 64, 257
    L, x = Layer(K, N, 5), make_x(M, K, 5)
    with torch.no_grad():
        alone = ops.linear(x, L.W, L.b, (L.gamma, L.beta, EPS), True)
    main = (x, L, dict(bias=True, ln=True, relu=True))
    check(alone, *main)
    others = []
    for i, (m, ep) in enumerate(((0, dict(bias=True)),
                                 (1, dict(bias=True, ln=True, dot=True)),
                                 (129, dict(relu=True, scale=scalar(-1.7), addend=full_addend(129, N, 5))),
                                 (300, dict(bias=True, scale=scalar(0.6), addend=row_addend(N, 5), bcast=True)))):
        others.append((make_x(m, K, 50 + i), Layer(K, N, 50 + i), ep))
    single = [launch(*o) for o in others]
    for o, got in zip(others[1:], single[1:]):
        check(got, *o)
    for pos in (0, 2, 4):
        order = others[:pos] + [main] + others[pos:]
        want = single[:pos] + [alone] + single[pos:]
        bufs = [sent(o[0].shape[0] + GUARD, 1 if o[2].get("dot") else N) for o in order]
        ops.linear_grouped([group(o[0], o[1], b[:o[0].shape[0]], o[2]) for o, b in zip(order, bufs)], K, N)
        for i, (o, b, w) in enumerate(zip(order, bufs, want)):
            m = o[0].shape[0]
            assert same_bits(b[:m], w), (pos, i)
            assert is_sent(b[m:]), (pos, i)


def test_launch_without_rows_touches_nothing(hiplib):
    from ocn_amd import ops
    K, N = 48, 64
    xb = sent(4, K)
    bufs = [sent(4, N), sent(4, N), sent(4, 1)]
    eps = [dict(bias=True), dict(ln=True, relu=True, scale=scalar(0.6)), dict(bias=True, dot=True)]
    ops.linear_grouped([group(xb[:0], Layer(K, N, 6 + i), b[:0], ep) for i, (b, ep) in enumerate(zip(bufs, eps))], K, N)
    torch.cuda.synchronize()
    assert all(is_sent(b) for b in bufs) and is_sent(xb)


# ---- 5. a row's result does not depend on where the row stands ---------------------------------------------------------------------
@pytest.mark.parametrize("M", [129, 257])
@pytest.mark.parametrize("K,N", [(48, 64), (80, 256)])
def test_row_independence_under_roll(hiplib, M, K, N):
    L, x = Layer(K, N, 7), make_x(M, K, 7)
    xr = x.roll(37, 0).contiguous()
    for ep in (dict(bias=True, relu=True), dict(bias=True, ln=True, relu=True, dot=True)):
        a, b = launch(x, L, ep), launch(xr, L, ep)
        assert same_bits(b.roll(-37, 0), a), ep                             # other tile, other wave, next to the clamped tail rows


# ---- 6. row_range ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ranged(hiplib):
    """M = 300 at (64, 64): the unranged outputs every range is compared with."""
    K, N, M = 64, 64, RANGE_M
    L, x = Layer(K, N, 8), make_x(M, K, 8)
    ep_store = dict(bias=True, relu=True, scale=scalar(-1.7), addend=full_addend(M, N, 8))
    ep_dot = dict(bias=True, ln=True, relu=True, dot=True)
    full_store, full_dot = launch(x, L, ep_store), launch(x, L, ep_dot)
    check(full_store, x, L, ep_store)
    check(full_dot, x, L, ep_dot)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(8)).to(DEV)
    return dict(K=K, N=N, M=M, L=L, x=x, ep_store=ep_store, ep_dot=ep_dot, full_store=full_store, full_dot=full_dot, perm=perm)


@pytest.mark.parametrize("rng", RANGES, ids=lambda r: f"{r[0]}_{r[1]}")
def test_row_range_stores_only_its_rows(ranged, rng):
    from ocn_amd import ops
    c = ranged
    M, N = c["M"], c["N"]
    lo, hi = clamp(rng, M)
    r = dev_range(rng)
    # stored Y: the right half of a [M, 2N] buffer
    buf, want = sent(M + GUARD, 2 * N), sent(M + GUARD, 2 * N)
    ops.linear_grouped([group(c["x"], c["L"], buf[:M, N:], c["ep_store"], row_range=r)], c["K"], N)
    want[lo:hi, N:] = c["full_store"][lo:hi]
    assert same_bits(buf, want)
    # dot
    buf, want = sent(M + GUARD, 1), sent(M + GUARD, 1)
    ops.linear_grouped([group(c["x"], c["L"], buf[:M], c["ep_dot"], row_range=r)], c["K"], N)
    want[lo:hi] = c["full_dot"][lo:hi]
    assert same_bits(buf, want)
    # dot through a row map: only y[map[row]] of the rows in range
    buf, want = sent(M + GUARD, 1), sent(M + GUARD, 1)
    ops.linear_grouped([group(c["x"], c["L"], buf[:M], c["ep_dot"], row_range=r, y_row_map=c["perm"])], c["K"], N)
    want[c["perm"][lo:hi]] = c["full_dot"][lo:hi]
    assert same_bits(buf, want)


# ---- 7. y_row_map without a range ----------------------------------------------------------------------------------------------------
def test_row_map_permutes_the_dot_output(ranged):
    from ocn_amd import ops
    c = ranged
    L, x, perm = c["L"], c["x"], c["perm"]
    got = launch(x, L, c["ep_dot"], y_row_map=perm)
    assert same_bits(got[perm], c["full_dot"])
    with torch.no_grad():
        plain = ops.linear(x, L.W, L.b, (L.gamma, L.beta, EPS), True, (L.dotw, L.dotb))
        mapped = ops.linear(x, L.W, L.b, (L.gamma, L.beta, EPS), True, (L.dotw, L.dotb), y_row_map=perm)
    assert plain.shape == mapped.shape == (c["M"], 1)
    assert same_bits(plain, c["full_dot"]) and same_bits(mapped[perm], plain)


# ---- 8. linear_t -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N_in,K_out", [(1, 16, 32), (129, 48, 128), (257, 256, 256), (300, 64, 32)])
def test_linear_t_against_fp64(hiplib, M, N_in, K_out):
    from ocn_amd import ops
    g = torch.Generator().manual_seed(M + N_in)
    gy = make_x(M, N_in, 9)
    W = (torch.randn(N_in, K_out, generator=g) * (0.5 + torch.rand(N_in, 1, generator=g))).to(DEV)
    assert ops.linear_ok_t(gy, W)
    got = ops.linear_t(gy, W)
    exact = gy.double() @ W.double()
    err, err32 = (got.double() - exact).abs().max().item(), ((gy @ W).double() - exact).abs().max().item()
    assert got.shape == (M, K_out) and err <= max(2.0 * err32, 2e-7 * exact.abs().max().item()), (err, err32)
    if M == 129:                                                            # a column slice of a wider gradient buffer
        wide = sent(M, N_in + 8)
        wide[:, 4:4 + N_in] = gy
        assert not wide[:, 4:4 + N_in].is_contiguous() and same_bits(ops.linear_t(wide[:, 4:4 + N_in], W), got)


def test_linear_ok_t_refuses_what_the_kernel_does_not_take(hiplib):
    from ocn_amd import ops
    z = partial(torch.zeros, device=DEV)
    assert ops.linear_ok_t(z(5, 64), z(64, 32))
    assert not ops.linear_ok_t(z(5, 64), z(64, 48))                         # K_out outside the kernel's widths
    assert not ops.linear_ok_t(z(5, 24), z(24, 32))                         # N_in no multiple of the k step
    assert not ops.linear_ok_t(z(5, 48), z(64, 32))                         # shapes that do not multiply


# ---- 9. the panel cache follows the weight -------------------------------------------------------------------------------------------
def _follows(x, w, b, got):
    """``got`` is the product with the values ``w`` holds now: the bits of a fresh tensor's run, and the fp32-GEMM bar."""
    from ocn_amd import ops
    fresh = ops.linear(x, w.detach().clone(), b)
    exact = F.linear(x.double(), w.double(), b.double())
    err, err32 = (got.double() - exact).abs().max().item(), (F.linear(x, w, b).double() - exact).abs().max().item()
    return same_bits(got, fresh) and err <= max(2.0 * err32, 2e-7 * exact.abs().max().item())


def test_panel_cache_follows_a_repointed_weight(hiplib):
    from ocn_amd import ops
    M, K, N = 33, 48, 64
    x = make_x(M, K, 10)
    g = torch.Generator().manual_seed(10)
    lin = torch.nn.Linear(K, N).to(DEV)
    with torch.no_grad():
        first = ops.linear(x, lin.weight, lin.bias)
        assert _follows(x, lin.weight, lin.bias, first)
        lin.weight.data = torch.randn(N, K, generator=g).to(DEV)          # same Parameter object, other storage
        second = ops.linear(x, lin.weight, lin.bias)
        assert _follows(x, lin.weight, lin.bias, second) and not torch.equal(first, second)


def test_panel_cache_survives_modules_that_come_and_go(hiplib):
    """A module is deleted and another of the same shape created: its weight may get the same address and the same ``id``."""
    from ocn_amd import ops
    M, K, N = 33, 48, 64
    x = make_x(M, K, 11)
    seen = []
    with torch.no_grad():
        for i in range(6):
            torch.manual_seed(100 + i)
            lin = torch.nn.Linear(K, N).to(DEV)
            got = ops.linear(x, lin.weight, lin.bias)
            assert _follows(x, lin.weight, lin.bias, got), i
            assert all(not torch.equal(got, s) for s in seen), i
            seen.append(got)
            del lin


# ---- 10. fill_rows -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [4, 32, 256])
def test_fill_rows_writes_its_range_only(hiplib, width):
    from ocn_amd import ops
    M = RANGE_M
    vec = torch.randn(width, generator=torch.Generator().manual_seed(width)).to(DEV)
    for rng in RANGES:
        lo, hi = clamp(rng, M)
        for half in (0, 1):
            buf, want = sent(M + GUARD, 2 * width), sent(M + GUARD, 2 * width)
            ops.fill_rows(buf[:M, half * width:(half + 1) * width], vec, dev_range(rng))
            want[lo:hi, half * width:(half + 1) * width] = vec
            assert same_bits(buf, want), (rng, half)


# ---- 11. the fused heads against fp64 where test_heads_product_accuracy does not go ------------------------------------------------
@pytest.mark.parametrize("H,ln", [(128, True), (128, False), (256, False)])
def test_heads_product_accuracy_other_widths(hiplib, H, ln):
    """``test_heads_product_accuracy`` (H = 256, LayerNorm) at the other widths / without LayerNorm, same weights recipe, same
    inputs recipe at scale 1.0, same bar; B = 257 (a ragged last tile) in both forms of the kernel."""
    from ocn_amd import ops
    from ocn_amd.model import predictor_dict
    B = 257
    torch.manual_seed(11)
    pred = partial(predictor_dict["cn5"], cndeg=-1)(H, H, 1, 3, 0.0, 0.0, ln).to(DEV).eval()
    with torch.no_grad():
        for p in pred.parameters():
            p.mul_(1.0 + 0.5 * torch.rand_like(p))
    x1, x2, xij = (torch.randn(B, H, device=DEV) * 1.0 for _ in range(3))
    x1[::3] *= 1e-3
    x2[:, ::5] *= 1e3
    x1[7].zero_()
    with torch.no_grad():
        p64 = copy.deepcopy(pred).double()
        a = torch.sigmoid(p64.alpha).cumprod(-1)

        def head(m, dt):
            z = a.to(dt)[0] * m.xcn1lin(x1.to(dt)) + a.to(dt)[1] * m.xcn2lin(x2.to(dt)) + m.beta.to(dt) * m.xijlin(xij.to(dt))
            return m.lin(z)
        ref64 = head(p64, torch.float64)
        ref32 = head(pred, torch.float32).double()
    e_32 = (ref32 - ref64).abs()
    prev = ops.heads_small_batch()
    try:
        for bound in (0, 1 << 40):                                          # 128 candidates per workgroup | 32
            ops.heads_small_batch(bound)
            with torch.no_grad():
                got = pred._heads_fused(x1.contiguous(), x2.contiguous(), xij.contiguous(), None).double()
            e_got = (got - ref64).abs()
            assert got.shape == (B, 1) and torch.isfinite(got).all()
            assert e_got.max() <= 1.5 * e_32.max() + 1e-7 * ref64.abs().max(), (bound, e_got.max().item(), e_32.max().item())
            assert e_got.pow(2).mean().sqrt() <= 1.5 * e_32.pow(2).mean().sqrt() + 1e-8, \
                (bound, e_got.pow(2).mean().sqrt().item(), e_32.pow(2).mean().sqrt().item())
    finally:
        ops.heads_small_batch(prev)
