"""The three AdamW launches of csrc/softmax.hip -- mk_adamw, mk_adamw_multi, mk_adamw_multi_dev -- and the FusedAdamW
methods that issue them, against the float64 restatement and the elementwise bounds of tests/adamw_ref.py (derived from the
kernel source, checked on the CPU by tests/test_adamw_ref_cpu.py; nothing here is fitted to what the GPU returns).

Every kernel-level launch works on param / master / m / v / grad placed in the MIDDLE of larger buffers at a 16-byte
aligned offset, between pads filled with a NaN bit pattern.  After the launch (Item.check):
  - the pads of all five buffers are bit-unchanged (a write outside the tensor, on either side);
  - grad is bit-unchanged;
  - m, v and master are inside E_m, E_v, E_w of step64 on every element (a pad that was READ shows as NaN);
  - param is master rounded to the element type, bit for bit (param starts from a value no update produces, so a store
    that never happened shows even where the rounding would hide the step);
  - the planted elements with g = m = v = 0 keep m = v = 0 exactly and only decay.
Sizes, lists and hyper-parameter cases come from adamw_ref; the slice size of the multi-tensor kernel is read from the
library (mk_adamw_chunk)."""
import ctypes

import pytest
import torch

import adamw_ref as R
from macaw_llm_amd import lib as _L
from macaw_llm_amd import ops
from macaw_llm_amd.optim import FusedAdamW

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DT_ID = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
PAD = 64                                       # elements on either side: 128 or 256 bytes, a multiple of 16
# NaN bit patterns with a recognisable payload
SENTINEL = {torch.float32: (torch.int32, 0x7FC00123), torch.bfloat16: (torch.int16, 0x7FC1),
            torch.float16: (torch.int16, 0x7E01)}
CHUNK = int(_L.load().mk_adamw_chunk())        # the library loads without a GPU
SIZES_MULTI = R.SIZES_MULTI(CHUNK)
LISTS = R.LISTS(CHUNK)
CASES = list(R.HYPER_CASES)


def _bits(t):
    return t.view(SENTINEL[t.dtype][0])


class Padded:
    """`values` in the middle of a sentinel-filled device buffer"""

    def __init__(self, values, dev):
        n = values.numel()
        self.n = n
        self.full = torch.empty(n + 2 * PAD, dtype=values.dtype, device=dev)
        _bits(self.full).fill_(SENTINEL[values.dtype][1])
        self.t = self.full[PAD:PAD + n]
        self.t.copy_(values)
        assert (self.full.data_ptr() + PAD * values.element_size()) % 16 == 0

    def ptr(self):
        return self.full.data_ptr() + PAD * self.full.element_size()

    def pads_intact(self):
        b = _bits(self.full).cpu()
        s = SENTINEL[self.full.dtype][1]
        return bool((b[:PAD] == s).all()) and bool((b[PAD + self.n:] == s).all())


class Item:
    """one tensor's five padded buffers for hyper case `case`, and the CPU copies of what went in"""
    NAMES = ("param", "master", "m", "v", "grad")

    def __init__(self, case, n, dtype, dev, seed=0):
        self.case, self.n, self.dtype = case, n, dtype
        self.w, self.m0, self.v0, self.g = R.make_state(case, n, dtype, seed)
        self.param = Padded(torch.full((n,), 3.0, dtype=dtype), dev)       # no update of w ~ 0.02 lands on 3
        self.master = Padded(self.w, dev)
        self.m = Padded(self.m0, dev)
        self.v = Padded(self.v0, dev)
        self.grad = Padded(self.g, dev)

    def row(self):
        return [getattr(self, k).ptr() for k in self.NAMES] + [self.n]

    def reference(self):
        return R.step64(self.w, self.m0, self.v0, self.g, *R.hyper_args(R.HYPER_CASES[self.case]))

    def state(self):
        return tuple(getattr(self, k).t.cpu() for k in ("param", "master", "m", "v"))

    def check(self, what):
        for k in self.NAMES:
            assert getattr(self, k).pads_intact(), f"{what}: a pad of {k} was written"
        assert torch.equal(_bits(self.grad.t.cpu()), _bits(self.g)), f"{what}: the gradient was written"
        param, master, m, v = self.state()
        ref = self.reference()
        rm = R.assert_within(m, ref.m, ref.E_m, f"{what} m")
        rv = R.assert_within(v, ref.v, ref.E_v, f"{what} v")
        rw = R.assert_within(master, ref.w, ref.E_w, f"{what} master")
        print(f"{what}: worst err / bound  m {rm:.3f}  v {rv:.3f}  w {rw:.3f}")
        assert torch.equal(_bits(param), _bits(master.to(self.dtype))), f"{what}: param is not master rounded to {self.dtype}"
        z = R.zero_run(self.n)
        assert not m[z].any() and not v[z].any(), f"{what}: a moment left zero without a gradient"
        return param, master, m, v


def _untouched(item, what):
    """an item no block owns (an empty tensor, or one left out of the launch)"""
    for k in Item.NAMES:
        assert getattr(item, k).pads_intact(), f"{what}: a pad of {k} was written"


def _single(item, cap=0):
    h = R.HYPER_CASES[item.case]
    lib = _L.load()
    prev = lib.mk_adamw_set_max_blocks(cap) if cap else 0
    try:
        assert prev == 0
        ops.adamw_(item.param.t, item.master.t, item.m.t, item.v.t, item.grad.t, *R.hyper_args(h))
        torch.cuda.synchronize()
    finally:
        if cap:
            assert lib.mk_adamw_set_max_blocks(0) == cap


def _table(items, dev):
    """the device table as optim.py builds it: 6 int64 per item, then the chunk prefix"""
    rows = [x for it in items for x in it.row()]
    starts = R.chunk_starts([it.n for it in items], CHUNK)
    return torch.tensor(rows + starts, dtype=torch.int64).to(dev), starts[-1]


def _multi(items, dev, dev_hyper=False):
    h = R.HYPER_CASES[items[0].case]
    lib = _L.load()
    n = len(items)
    devt, chunks = _table(items, dev)
    st = torch.cuda.current_stream(dev).cuda_stream
    dtc = ops._DT[items[0].dtype]
    if dev_hyper:
        bc = (ctypes.c_float * 2)()
        _L.check(lib.mk_adamw_bias_correction(h.b1, h.b2, h.step, bc), "mk_adamw_bias_correction")
        hyper = torch.tensor([h.lr, float(bc[0]), float(bc[1]), h.gs], dtype=torch.float32).to(dev)
        _L.check(lib.mk_adamw_multi_dev(devt.data_ptr(), devt.data_ptr() + 6 * n * 8, n, chunks, h.b1, h.b2, h.eps, h.wd,
                                        hyper.data_ptr(), dtc, st), "mk_adamw_multi_dev")
    else:
        _L.check(lib.mk_adamw_multi(devt.data_ptr(), devt.data_ptr() + 6 * n * 8, n, chunks, h.lr, h.b1, h.b2, h.eps,
                                    h.wd, h.step, h.gs, dtc, st), "mk_adamw_multi")
    torch.cuda.synchronize()


def _items(case, sizes, dtype, dev):
    return [Item(case, n, dtype, dev, seed=i) for i, n in enumerate(sizes)]


def _same_bits(a, b, what):
    for name, x, y in zip(("param", "master", "m", "v"), a, b):
        assert torch.equal(_bits(x), _bits(y)), f"{what}: {name} differs in {int((_bits(x) != _bits(y)).sum())} of {x.numel()}"


# ---- mk_adamw -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("n,cap", R.SIZES_SINGLE, ids=[f"n{n}_cap{c}" for n, c in R.SIZES_SINGLE])
def test_single_every_size(dev, n, cap, dtype):
    it = Item("eps_gs", n, dtype, dev)
    _single(it, cap)
    it.check(f"mk_adamw n={n} cap={cap} {DT_ID[dtype]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("case", CASES)
def test_single_every_hyper_case(dev, case, dtype):
    it = Item(case, 10242, dtype, dev)
    _single(it)
    it.check(f"mk_adamw {case} {DT_ID[dtype]}")


# ---- mk_adamw_multi -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("n", SIZES_MULTI)
def test_multi_every_size(dev, n, dtype):
    it = Item("eps_gs", n, dtype, dev)
    _multi([it], dev)
    it.check(f"mk_adamw_multi n={n} {DT_ID[dtype]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("name", list(LISTS))
def test_multi_every_list(dev, name, dtype):
    items = _items("eps_gs", LISTS[name], dtype, dev)
    bystander = Item("eps_gs", 1031, dtype, dev, seed=99)               # allocated beside them, not in the table
    _multi(items, dev)
    for i, it in enumerate(items):
        if it.n:
            it.check(f"mk_adamw_multi list {name} item {i} (n={it.n}) {DT_ID[dtype]}")
        else:
            _untouched(it, f"list {name} empty item {i}")
    _untouched(bystander, f"list {name} bystander")
    assert torch.equal(bystander.master.t.cpu(), bystander.w) and torch.equal(bystander.m.t.cpu(), bystander.m0)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("case", CASES)
def test_multi_every_hyper_case(dev, case, dtype):
    items = _items(case, LISTS["seventeen"], dtype, dev)
    _multi(items, dev)
    for i, it in enumerate(items):
        it.check(f"mk_adamw_multi {case} item {i} (n={it.n}) {DT_ID[dtype]}")


# ---- mk_adamw_multi_dev ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
@pytest.mark.parametrize("case", ["eps_gs", "unscale_settled"])
def test_multi_dev_is_multi_bit_for_bit(dev, case, dtype):
    """the per-step scalars from device memory, the corrections from mk_adamw_bias_correction: the same bits as the host
    form at the same step, and inside the bounds; grad_scale != 1 in both cases"""
    assert R.HYPER_CASES[case].gs != 1.0
    host = _items(case, LISTS["seventeen"], dtype, dev)
    devi = _items(case, LISTS["seventeen"], dtype, dev)
    _multi(host, dev)
    _multi(devi, dev, dev_hyper=True)
    for i, (a, b) in enumerate(zip(host, devi)):
        what = f"mk_adamw_multi_dev {case} item {i} (n={a.n}) {DT_ID[dtype]}"
        _same_bits(a.state(), b.check(what), what)


# ---- across forms ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_single_and_multi_agree_bit_for_bit(dev, dtype):
    """the shard path (mk_adamw) and the bucket path (mk_adamw_multi) are interchangeable in checkpoints: identical inputs
    give identical bits in every element type, vector bodies and scalar tails alike"""
    sizes = LISTS["seventeen"] + [10242]
    one = _items("eps_gs", sizes, dtype, dev)
    many = _items("eps_gs", sizes, dtype, dev)
    for it in one:
        _single(it)
    _multi(many, dev)
    for i, (a, b) in enumerate(zip(one, many)):
        _same_bits(a.state(), b.state(), f"single vs multi item {i} (n={a.n}) {DT_ID[dtype]}")


# ---- FusedAdamW -----------------------------------------------------------------------------------------------------
class Trajectory:
    """the float64 run of one tensor with the bounds accumulated step by step (step64's `err`)"""

    def __init__(self, w):
        n = w.numel()
        self.s = R.Step(w.double().cpu().reshape(-1), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
                        torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64),
                        torch.zeros(n, dtype=torch.float64))

    def step(self, g, lr, b1, b2, eps, wd, step, gs):
        s = self.s
        self.s = R.step64(s.w, s.m, s.v, g.cpu().reshape(-1), lr, b1, b2, eps, wd, step, gs, err=(s.E_w, s.E_m, s.E_v))

    def check(self, slot, param, what):
        master, m, v = (t.cpu().reshape(-1) for t in slot)
        s = self.s
        R.assert_within(m, s.m, s.E_m, f"{what} m")
        R.assert_within(v, s.v, s.E_v, f"{what} v")
        R.assert_within(master, s.w, s.E_w, f"{what} master")
        p = param.detach().cpu().reshape(-1)
        assert torch.equal(_bits(p), _bits(master.to(p.dtype))), f"{what}: param is not master rounded"


def _grad(shape, dtype, gen, sigma=1e-3):
    return (torch.randn(shape, generator=gen, dtype=torch.float64) * sigma).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_step_follows_each_parameter_group(dev, dtype):
    """step() with two groups that differ in lr, betas, eps and weight_decay: every parameter follows ITS group's values
    for three steps (bounds accumulated per step); eps is of the size of sqrt(v), so a swapped eps shows"""
    gen = torch.Generator().manual_seed(11)
    shapes = [(1031,), (CHUNK + 1,), (7,), (3, 684)]
    base = [(torch.randn(s, generator=gen) * 0.02).to(dtype) for s in shapes]
    ps = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    hp = [dict(lr=1e-2, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.1),
          dict(lr=3e-3, betas=(0.8, 0.999), eps=1e-3, weight_decay=0.0)]
    opt = FusedAdamW([dict(params=ps[:2], **hp[0]), dict(params=ps[2:], **hp[1])])
    traj = [Trajectory(b) for b in base]
    for step in (1, 2, 3):
        grads = [_grad(s, dtype, gen) for s in shapes]
        for p, g in zip(ps, grads):
            p.grad = g.to(dev)
        opt.step(grad_scale=0.5)
        torch.cuda.synchronize()
        assert opt.step_count == step
        for i, (p, g, t) in enumerate(zip(ps, grads, traj)):
            h = hp[i // 2]
            t.step(g, h["lr"], h["betas"][0], h["betas"][1], h["eps"], h["weight_decay"], step, 0.5)
            t.check(opt.state[p], p.data, f"step() group {i // 2} parameter {i} step {step} {DT_ID[dtype]}")
            assert torch.equal(_bits(p.grad.cpu()), _bits(g))


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_step_buckets_host_scalars_and_device_scalars(dev, dtype):
    """two flat buckets for six steps, lr and grad_scale new at every step: the host-scalar launch and the dev_hyper launch
    (update_hyper's four pinned slots are each reused, and nothing synchronises between the steps) agree bit for bit at
    every step, and both stay inside the accumulated bounds"""
    gen = torch.Generator().manual_seed(23)
    sizes = [2 * CHUNK + 1031, CHUNK + 1]
    base = [(torch.randn(n, generator=gen) * 0.02).to(dtype) for n in sizes]
    lrs = [1e-3, 2e-3, 5e-4, 1.5e-3, 7e-4, 3e-3]
    scales = [1.0, 0.37, 0.5, 0.81, 2.0 ** -3, 0.9]
    grads = [[_grad((n,), dtype, gen) for n in sizes] for _ in lrs]
    assert len(lrs) > FusedAdamW._HYPER_SLOTS

    def run(dev_hyper):
        ws = [b.clone().to(dev) for b in base]
        gs = [torch.zeros_like(w) for w in ws]
        opt = FusedAdamW([torch.nn.Parameter(torch.zeros(8, device=dev))], lr=1e-3, betas=(0.9, 0.95), eps=1e-3,
                         weight_decay=0.1)
        items = [((i, 0, w.numel()), w, g) for i, (w, g) in enumerate(zip(ws, gs))]
        seen = []
        for k, (lr, scale) in enumerate(zip(lrs, scales)):
            for g, src in zip(gs, grads[k]):
                g.copy_(src.to(dev))
            opt.step_count += 1
            opt.lr = lr
            if dev_hyper:
                opt.update_hyper(dev, scale)
                opt.step_buckets(items, dev_hyper=True)
            else:
                opt.step_buckets(items, scale)
            seen.append([(w.clone(),) + tuple(t.clone() for t in opt.state[key]) for key, w, _ in items])
        torch.cuda.synchronize()
        return [[tuple(t.cpu() for t in b) for b in s] for s in seen]

    host, devh = run(False), run(True)
    traj = [Trajectory(b) for b in base]
    for k, (lr, scale) in enumerate(zip(lrs, scales)):
        for b in range(len(sizes)):
            what = f"step_buckets bucket {b} step {k + 1} {DT_ID[dtype]}"
            _same_bits(host[k][b], devh[k][b], what)
            traj[b].step(grads[k][b], lr, 0.9, 0.95, 1e-3, 0.1, k + 1, scale)
            for got in (host[k][b], devh[k][b]):
                traj[b].check(got[1:], got[0], what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_step_params_dev_is_step_params_bit_for_bit(dev, dtype):
    """the graph form run eagerly (prepare_graph, update_hyper, step_params_dev) against step_params, two steps"""
    gen = torch.Generator().manual_seed(31)
    shapes = [(1031,), (CHUNK + 1,), (7,), (3, 684), (2048,)]
    base = [(torch.randn(s, generator=gen) * 0.02).to(dtype) for s in shapes]
    pa = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    pb = [torch.nn.Parameter(b.clone().to(dev)) for b in base]
    kw = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-3, weight_decay=0.1)
    oa, ob = FusedAdamW(pa, **kw), FusedAdamW(pb, **kw)
    ob.prepare_graph(pb)
    traj = [Trajectory(b) for b in base]
    for step, scale in ((1, 0.37), (2, 0.81)):
        grads = [_grad(s, dtype, gen) for s in shapes]
        for p, q, g in zip(pa, pb, grads):
            p.grad, q.grad = g.to(dev), g.to(dev)
        oa.step_count += 1
        oa.step_params(pa, scale)
        ob.step_count += 1
        ob.update_hyper(dev, scale)
        ob.step_params_dev(pb)
        torch.cuda.synchronize()
        for i, (p, q, g) in enumerate(zip(pa, pb, grads)):
            what = f"step_params_dev parameter {i} step {step} {DT_ID[dtype]}"
            a = (p.data.cpu(),) + tuple(t.cpu() for t in oa.state[p])
            b = (q.data.cpu(),) + tuple(t.cpu() for t in ob.state[q])
            _same_bits(a, b, what)
            traj[i].step(g, kw["lr"], 0.9, 0.95, 1e-3, 0.1, step, scale)
            traj[i].check(ob.state[q], q.data, what)


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_ID.get)
def test_step_shard_is_step_param_bit_for_bit(dev, dtype):
    """a ZeRO-1 slice of a flat buffer against a parameter that holds the same values; the rest of the buffer stays"""
    gen = torch.Generator().manual_seed(41)
    total, lo, n = 3 * CHUNK, 1024 + 8, CHUNK + 1031
    flat = (torch.randn(total, generator=gen) * 0.02).to(dtype)
    kw = dict(lr=2e-3, betas=(0.9, 0.95), eps=1e-3, weight_decay=0.1)
    W = flat.clone().to(dev)
    oa = FusedAdamW([torch.nn.Parameter(torch.zeros(8, device=dev))], **kw)
    p = torch.nn.Parameter(flat[lo:lo + n].clone().to(dev))
    ob = FusedAdamW([p], **kw)
    traj = Trajectory(flat[lo:lo + n])
    key = ("flat", lo, n)
    for step, scale in ((1, 0.37), (2, 0.81)):
        g = _grad((n,), dtype, gen)
        oa.step_count = ob.step_count = step
        oa.step_shard(key, W[lo:lo + n], g.to(dev), scale)
        p.grad = g.to(dev)
        ob.step_param(p, scale)
        torch.cuda.synchronize()
        what = f"step_shard step {step} {DT_ID[dtype]}"
        a = (W[lo:lo + n].cpu(),) + tuple(t.cpu() for t in oa.state[key])
        b = (p.data.cpu(),) + tuple(t.cpu() for t in ob.state[p])
        _same_bits(a, b, what)
        traj.step(g, kw["lr"], 0.9, 0.95, 1e-3, 0.1, step, scale)
        traj.check(oa.state[key], W[lo:lo + n], what)
        out = W.cpu()
        assert torch.equal(_bits(out[:lo]), _bits(flat[:lo])) and torch.equal(_bits(out[lo + n:]), _bits(flat[lo + n:]))
