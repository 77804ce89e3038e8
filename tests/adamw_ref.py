"""A float64 restatement of the AdamW update of csrc/softmax.hip (adamw_kernel, adamw_multi_kernel), the elementwise
error bounds the kernels are held to, seven deliberately wrong variants, and the hyper-parameter / size / list tables that
tests/test_adamw_edges_gpu.py feeds the kernels and tests/test_adamw_ref_cpu.py feeds the restatement.  CPU only.

The update (torch.optim.AdamW: decoupled decay, bias-corrected moments, eps outside the square root):
    g' = g gs;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  w1 = w - lr wd w
    w' = w1 - lr (m' / bc1) / (sqrt(v' / bc2) + eps),   bc = 1 - b^step
step64 evaluates it in float64 from the fp32 state, the gradient widened exactly from its element type and the scalars
ROUNDED TO fp32 (what the C ABI receives), so the only differences left are the kernel's own fp32 roundings and the fp32
bias corrections the host computes with powf.

The bounds.  u = 2^-24 is the relative error of one correctly rounded fp32 operation.  A value that went through r
roundings is off by (1 + u)^r - 1 relative; every K below is TWICE the count r read from the kernel source, which covers
the higher-order terms and a division or square root that is faithful (1 ulp) instead of correctly rounded (1/2 ulp).
Contracting a product and a sum into an FMA only removes roundings.  Source, per element (the three vector
bodies and the two scalar tails are the same statements):
    gk = g * gscale                                            1 rounding
    m' = b1 * m + (1.f - b1) * gk                              b1 m: product, sum = 2;  the other addend: 1 - b1, gk,
                                                               product, sum = 4                               -> K_M = 2 * 4
    v' = b2 * v + (1.f - b2) * gk * gk                         b2 v: 2;  the other: 1 - b2, gk twice, two products,
                                                               sum = 6                                        -> K_V = 2 * 6
    wk -= lr * wd * wk                                         lr wd, (lr wd) w = 2 on the decay term         -> K_DECAY = 2 * 2
                                                               the subtraction: u |w1|
    wk -= lr * (m' * ib1) / (sqrtf(v' * ib2) + eps)            ib1 = 1 / bc1, m' ib1, lr (...), the division = 4;
                                                               ib2 = 1 / bc2 and v' ib2 sit under the square root, which
                                                               halves a relative error: 2 * 1/2 = 1;  sqrtf, + eps = 2
                                                                                                              -> K_UPD = 2 * 7
                                                               the subtraction: u |w'|
The errors of m' and v' reach w' through the update: E_m / bc1 times lr / den, and E_v / v' halved by the square root
(times sqrt / den <= 1, the share of the denominator the root has).  The host adds the error of its bias corrections:
1.f - powf(b, step) is within 2 u ABSOLUTE of the float64 value (powf within an ulp of a value below 1, i.e. u, and one
subtraction of a result below 1, u), which is 2 u / bc1 relative on 1 / bc1 and, halved by the root, u / bc2 on the
denominator: DELTA = 2 u / bc1 + u / bc2, relative to the update.

step64 also takes the error bounds of its INPUT state (err = (E_w, E_m, E_v) of the previous step) and carries them
through the same first-order propagation, so a run of several steps is held to bounds accumulated step by step around the
float64 trajectory.  Nothing here was fitted to what a GPU returned."""
import collections
import math

import numpy as np
import torch

U = 2.0 ** -24
K_M = 2 * 4          # see the module docstring for each count
K_V = 2 * 6
K_DECAY = 2 * 2
K_UPD = 2 * 7

Step = collections.namedtuple("Step", "w m v E_w E_m E_v")


def f32(x):
    """the value a C float argument receives, as a Python float"""
    return float(np.float32(x))


def bias_corrections64(b1, b2, step):
    """1 - b^step in float64 from the fp32-rounded betas"""
    return 1.0 - f32(b1) ** int(step), 1.0 - f32(b2) ** int(step)


def _f64(t):
    return torch.as_tensor(t).detach().cpu().to(torch.float64)


def step64(w, m, v, g, lr, b1, b2, eps, wd, step, gs, err=None):
    """one AdamW step in float64 and its elementwise bounds: Step(w', m', v', E_w, E_m, E_v), float64 tensors.
    err: bounds (E_w, E_m, E_v) on the INPUT state's distance from (w, m, v), propagated to first order."""
    w, m, v, g = _f64(w), _f64(m), _f64(v), _f64(g)
    lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, b1, b2, eps, wd, gs))
    bc1, bc2 = bias_corrections64(b1, b2, step)
    ew, em, ev = (_f64(e) for e in err) if err is not None else (0.0, 0.0, 0.0)
    gp = g * gs
    ma, mb = b1 * m, (1.0 - b1) * gp
    m1 = ma + mb
    E_m = K_M * U * (ma.abs() + mb.abs()) + b1 * em                  # 4 roundings at most on either addend
    va, vb = b2 * v, (1.0 - b2) * gp * gp
    v1 = va + vb
    E_v = K_V * U * (va + vb) + b2 * ev                              # 6 roundings at most; both addends are >= 0
    decay = lr * wd * w
    w1 = w - decay
    root = torch.sqrt(v1 / bc2)
    den = root + eps
    upd = lr * (m1 / bc1) / den
    w2 = w1 - upd
    delta = 2.0 * U / bc1 + U / bc2                                  # the host's fp32 bias corrections
    rel_root = torch.where(v1 > 0, 0.5 * E_v / torch.where(v1 > 0, v1, torch.ones_like(v1)), torch.zeros_like(v1))
    E_w = (abs(1.0 - lr * wd) * ew                                   # the input's own error, decayed like w
           + K_DECAY * U * decay.abs()                               # lr wd, (lr wd) w
           + U * (w1.abs() + w2.abs())                               # the two subtractions
           + lr / (bc1 * den) * E_m                                  # m' through lr / den
           + upd.abs() * (rel_root * root / den                      # v' through the square root
                          + K_UPD * U + delta))                      # 7 roundings of the update itself; the host's bc
    return Step(w2, m1, v1, E_w, E_m, E_v)


# ---- the same step with one plausible bug each ---------------------------------------------------------------------
BUGS = ("eps_inside_sqrt", "gs_missing_from_v", "bc1_for_both", "bc_at_previous_step", "l2_instead_of_decoupled",
        "decay_after_update", "update_from_old_m")


def _flagged(bug):
    """step64's values (no bounds) with `bug` switched on; bug = None is step64 itself (asserted on the CPU)"""
    assert bug is None or bug in BUGS

    def run(w, m, v, g, lr, b1, b2, eps, wd, step, gs):
        w, m, v, g = _f64(w), _f64(m), _f64(v), _f64(g)
        lr, b1, b2, eps, wd, gs = (f32(x) for x in (lr, b1, b2, eps, wd, gs))
        s = step - 1 if (bug == "bc_at_previous_step" and step > 1) else step
        bc1, bc2 = bias_corrections64(b1, b2, s)
        if bug == "bc1_for_both":
            bc2 = bc1
        gp = g * gs
        gm = gp + wd * w if bug == "l2_instead_of_decoupled" else gp
        gv = (g if bug == "gs_missing_from_v" else gp)
        gv = gv + wd * w if bug == "l2_instead_of_decoupled" else gv
        m1 = b1 * m + (1.0 - b1) * gm
        v1 = b2 * v + (1.0 - b2) * gv * gv
        mu = m if bug == "update_from_old_m" else m1
        if bug == "eps_inside_sqrt":
            den = torch.sqrt(v1 / bc2 + eps)
        else:
            den = torch.sqrt(v1 / bc2) + eps
        upd = lr * (mu / bc1) / den
        if bug == "l2_instead_of_decoupled":
            w2 = w - upd
        elif bug == "decay_after_update":
            w2 = w - upd
            w2 = w2 - lr * wd * w2
        else:
            w2 = (w - lr * wd * w) - upd
        return w2, m1, v1
    return run


mutants = {bug: _flagged(bug) for bug in BUGS}


def step32(w, m, v, g, lr, b1, b2, eps, wd, step, gs):
    """the kernel's statements in numpy float32, operation by operation and without FMA contraction (the most roundings
    a correct kernel can make), bias corrections with numpy's powf as the host computes them -> (w', m', v') float32"""
    f = np.float32
    w, m, v, g = (np.asarray(torch.as_tensor(t).detach().cpu().to(torch.float32).numpy(), dtype=f) for t in (w, m, v, g))
    lr, b1, b2, eps, wd, gs = (f(x) for x in (lr, b1, b2, eps, wd, gs))
    bc1 = f(1) - np.power(b1, f(step), dtype=f)
    bc2 = f(1) - np.power(b2, f(step), dtype=f)
    ib1, ib2 = f(1) / bc1, f(1) / bc2
    gk = g * gs
    m1 = b1 * m + (f(1) - b1) * gk
    v1 = b2 * v + (f(1) - b2) * gk * gk
    wk = w - lr * wd * w
    wk = wk - lr * (m1 * ib1) / (np.sqrt(v1 * ib2) + eps)
    for a in (m1, v1, wk):
        assert a.dtype == f
    return wk, m1, v1


# ---- hyper-parameter cases -----------------------------------------------------------------------------------------
# warm: the moments hold m ~ N(0, sigma^2), v = sigma^2 chi^2(1); fresh: zeros.  sigma_g is the spread of the gradient
# (before grad_scale), sigma the spread of the warm moments.
Hyper = collections.namedtuple("Hyper", "lr b1 b2 eps wd step gs sigma_g sigma warm")
HYPER_CASES = {
    # (i) the first step of a fresh optimizer
    "fresh": Hyper(1e-2, 0.9, 0.95, 1e-8, 0.1, 1, 1.0, 1.0, 1.0, False),
    # (ii) the benchmark's setting, long into a run
    "bench": Hyper(3e-5, 0.9, 0.999, 1e-8, 0.0, 1000, 1.0, 1.0, 1.0, True),
    # (iii) eps of the size of sqrt(v), a clipping scale: eps and grad_scale both move the result
    "eps_gs": Hyper(1e-3, 0.9, 0.999, 1e-3, 0.1, 2, 0.37, 1e-3, 1e-3, True),
    # (iv) loss-scale unscale: gradients of ~100, grad_scale 2^-16
    "unscale": Hyper(1e-4, 0.9, 0.95, 1e-8, 0.01, 7, 2.0 ** -16, 100.0, 100.0, True),
    # (iv) again with the moments where a run of such steps leaves them, at the scale of the UNSCALED gradient: the new
    # gradient then weighs as much as the old moments
    "unscale_settled": Hyper(1e-4, 0.9, 0.95, 1e-8, 0.01, 7, 2.0 ** -16, 100.0, 100.0 * 2.0 ** -16, True),
    # (v) both bias corrections are exactly 1.0 in fp32 (and in float64)
    "late": Hyper(3e-5, 0.9, 0.999, 1e-8, 0.1, 200000, 1.0, 1.0, 1.0, True),
}
HYPER_CASES = {k: h._replace(**{n: f32(getattr(h, n)) for n in ("lr", "b1", "b2", "eps", "wd", "gs")})
               for k, h in HYPER_CASES.items()}


def hyper_args(h):
    """the scalar arguments of step64 / step32 / a mutant"""
    return (h.lr, h.b1, h.b2, h.eps, h.wd, h.step, h.gs)


def zero_run(n):
    """the planted run of elements with g = m = v = 0 (unused embedding rows): up to 37 elements from n // 2 on, so that
    it crosses a 4-element vector and, in a long tensor, a thread's share; none in tensors shorter than 4"""
    k = min(37, n // 4)
    return slice(n // 2, n // 2 + k)


def make_state(case, n, dtype, seed=0):
    """(w, m, v) float32 and g in `dtype`, all on the CPU, for hyper case `case`: w ~ N(0, 0.02^2) as at initialisation,
    moments as the case says, the zero run planted"""
    h = HYPER_CASES[case]
    gen = torch.Generator().manual_seed(1000003 * seed + 7919 * n + sorted(HYPER_CASES).index(case))
    w = torch.randn(n, generator=gen) * 0.02
    g = (torch.randn(n, generator=gen, dtype=torch.float64) * h.sigma_g).to(dtype)
    if h.warm:
        m = (torch.randn(n, generator=gen, dtype=torch.float64) * h.sigma).float()
        v = (torch.randn(n, generator=gen, dtype=torch.float64) ** 2 * h.sigma ** 2).float()
    else:
        m, v = torch.zeros(n), torch.zeros(n)
    z = zero_run(n)
    g[z] = 0
    m[z] = 0
    v[z] = 0
    assert torch.isfinite(g.float()).all()
    return w, m, v, g


# ---- sizes ---------------------------------------------------------------------------------------------------------
SINGLE_THREADS, SINGLE_VEC, SINGLE_MAX_BLOCKS = 256, 4, 2048
# (n, grid cap): mk_adamw launches min((n / 8 + 255) / 256, 2048, cap) blocks of 256 threads, 4 elements per thread
SIZES_SINGLE = [(1, 0), (3, 0),                     # the scalar tail alone
                (4, 0), (7, 0),                     # one vector; one vector and a 3-element tail
                (2048, 0), (2051, 0),               # one block, two trips; the same with a 3-element tail
                (10242, 0),                         # 5 blocks, two grid-stride trips each, tail 2
                (5 * 2 ** 20 + 3, 0),               # beyond the 2048-block cap: three trips for some threads, two for others
                (4099, 1)]                          # mk_adamw_set_max_blocks(1): one block walks the tensor in 4 trips


def SIZES_MULTI(C):
    """element counts of a single-item mk_adamw_multi launch; C = mk_adamw_chunk().  The 1024 / 2048 edges are 256
    threads x 4 elements x 2 groups and do not move with C."""
    return [1, 3, 4,
            1020, 1024, 1028,                       # group 0 short of a full trip; exactly group 0; one vector of group 1
            1031,                                   # group 1 live for thread 0 only, and a 3-element tail
            2048, 2052, 3079,                       # one whole trip; a second trip of one vector; ragged second trip + tail
            C - 1, C, C + 1, C + 1031, 3 * C - 4]


def LISTS(C):
    """item lists for the block -> item binary search of the multi-tensor kernel"""
    return {"one": [2052],
            "two": [C + 1, 3],
            "single_element_in_the_middle": [1031, 1, 1028],
            # first and last slices of neighbours of every kind meet
            "seventeen": [3, C, 1, C + 1, 1031, 4, 3 * C - 4, 1020, 7, 2048, C - 1, 1024, 3079, 1, C + 1031, 2052, 1028],
            "empty_in_the_middle": [1031, 0, C + 1]}


def chunk_starts(sizes, C):
    """the chunk prefix optim.py builds: chunk_start[i] = sum over j < i of ceil(n_j / C)"""
    s = [0]
    for n in sizes:
        s.append(s[-1] + (n + C - 1) // C)
    return s


def branch_census(n, chunk=None, max_blocks=0):
    """which loop of the kernel each element of an n-element tensor takes, restated on the host.
    chunk = None: mk_adamw (adamw_kernel) under grid cap `max_blocks`; chunk = C: one item of mk_adamw_multi.
    Returns a dict: per element `tail` (bool), `trip` (iteration of its thread's loop), `group` (0 / 1; multi only, -1 in
    the tail), `block`; and the summaries `blocks`, `n_vector`, `n_tail`, `thread_trips` (the set of vector-loop trip counts
    over all launched threads) and, for multi, `two` (the set of outcomes of the `two` test over all vector iterations)."""
    i = np.arange(n, dtype=np.int64)
    if chunk is None:
        nb = min((n // 8 + SINGLE_THREADS - 1) // SINGLE_THREADS, SINGLE_MAX_BLOCKS)
        if max_blocks > 0:
            nb = min(nb, max_blocks)
        nb = max(nb, 1)
        T = nb * SINGLE_THREADS
        nch = n // SINGLE_VEC
        tail = i >= nch * SINGLE_VEC
        c = i // SINGLE_VEC
        thread = np.where(tail, i - nch * SINGLE_VEC, c % T)
        trip = np.where(tail, 0, c // T)
        t = np.arange(T, dtype=np.int64)
        trips = np.where(t < nch, (nch - t + T - 1) // T, 0)
        return dict(tail=tail, trip=trip, group=np.full(n, -1), block=thread // SINGLE_THREADS, blocks=nb,
                    n_vector=int(nch * SINGLE_VEC), n_tail=int(n - nch * SINGLE_VEC),
                    thread_trips=set(int(x) for x in np.unique(trips)), two=set())
    C = int(chunk)
    assert C % (2 * SINGLE_THREADS * SINGLE_VEC) == 0
    block = i // C
    off = i - block * C
    length = np.minimum(C, n - block * C)                           # of the element's slice
    vec = length // 4 * 4
    tail = off >= vec
    r = off // (SINGLE_THREADS * 4)                                 # which run of 1024 elements of the slice
    trip = np.where(tail, (off - vec) // SINGLE_THREADS, r // 2)
    group = np.where(tail, -1, r % 2)
    two, thread_trips = set(), set()
    nblocks = (n + C - 1) // C
    for b in sorted({0, nblocks - 1} if nblocks else ()):           # every slice but the last is a full one
        L = min(C, n - b * C)
        vend = L // 4 * 4
        i0 = np.arange(0, vend, 4, dtype=np.int64)
        i0 = i0[(i0 // 1024) % 2 == 0]                              # the iterations: group-0 starts
        two |= set(bool(x) for x in np.unique(i0 + 1024 < vend))
        t4 = np.arange(SINGLE_THREADS, dtype=np.int64) * 4
        thread_trips |= set(int(x) for x in np.unique(np.where(t4 < vend, (vend - t4 + 2047) // 2048, 0)))
    return dict(tail=tail, trip=trip, group=group, block=block, blocks=nblocks, n_vector=int((~tail).sum()),
                n_tail=int(tail.sum()), thread_trips=thread_trips, two=two)


def assert_within(got, ref, bound, what):
    """every element of `got` finite and within `bound` of `ref` (float64 tensors); the message names the worst element"""
    got, ref, bound = _f64(got).reshape(-1), _f64(ref).reshape(-1), _f64(bound).reshape(-1)
    assert got.shape == ref.shape == bound.shape, f"{what}: {tuple(got.shape)} against {tuple(ref.shape)}"
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all(), f"{what}: the reference itself is not finite"
    if got.numel() == 0:
        return 0.0
    bad = (~torch.isfinite(got)).nonzero()
    assert bad.numel() == 0, f"{what}: {bad.numel()} non-finite values, first at {int(bad[0])}"
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    i = int(ratio.argmax())
    assert bool((err <= bound).all()), (f"{what}: {int((err > bound).sum())} of {err.numel()} outside the bound; worst at {i}: "
                                        f"got {float(got[i]):.9g}, ref {float(ref[i]):.9g}, err {float(err[i]):.3e} > "
                                        f"{float(bound[i]):.3e}")
    return float(ratio[i])


def exceeds(got, ref, bound):
    """how many elements of a (mutant's) result lie outside the bound"""
    return int(((_f64(got) - _f64(ref)).abs() > _f64(bound)).sum())
