"""GPU: per-request sampling -- ops.sample_rows_table / ops.decode_emit_sample_table (csrc/sample.hip) and
generate(sampling_params=[...]).

The oracle is the project's SCALAR kernels on the same rows (ops.argmax_rows, ops.sample_rows, ops.sample_rows_warp),
which this table form leaves untouched and which tests/test_sampling_gpu.py and tests/test_warpers_gpu.py pin to their
restatements: row r of a table launch equals the scalar op on a [stream_r + 1, pitch] tensor whose last row is that
logits row, called with the record's values, seed and step, output stream_r.  Equality is exact, so no case is left out.
The records fed to the oracle are read back from the table's device bytes."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import sampling_params_ref as R  # noqa: E402
from golden_util import load_case  # noqa: E402
from oracle import configs  # noqa: E402
from test_sampling_gpu import _Spy, _ids, _kw, _small_llama  # noqa: E402
from warpers_ref import OFF, logits_host  # noqa: E402

from macaw_llm_amd import lib as L  # noqa: E402
from macaw_llm_amd import modeling as Mo  # noqa: E402
from macaw_llm_amd import ops  # noqa: E402

TDT = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NAN, NINF = float("nan"), float("-inf")


@pytest.fixture(autouse=True)
def _restore_switches():
    ops.clear_fp8_cache()
    yield
    Mo.AUTO_FUSE = True
    Mo.DECODE_WEIGHTS[0] = None
    Mo.KV_CACHE[0] = None
    Mo.SAMPLING_PARAMS[0] = None
    ops.clear_fp8_cache()


def _records(table):
    """the records of an ops.SampleTable as the device holds them"""
    raw = table.records.cpu()
    return [R.unpack(raw[r].numpy().tobytes()) for r in range(table.rows)]


def _scalar(x, r, V, rec, step):
    """the oracle: what the scalar kernels select for row r of x [rows, pitch] under the (unpacked) record"""
    if rec["mode"] != 1:
        return int(ops.argmax_rows(x[r:r + 1, :V], V))
    s = rec["stream"]
    buf = torch.zeros((s + 1, x.shape[1]), dtype=x.dtype, device=x.device)
    buf[s] = x[r]
    args = (rec["temperature"], rec["top_k"], rec["top_p"], rec["seed"])
    w = R.warpers(rec)
    if w == OFF:                                                          # what the scalar API selects
        out = ops.sample_rows(buf[:, :V], V, *args, step=step)
    else:
        out = ops.sample_rows_warp(buf[:, :V], V, *args, *w, step=step)
    return int(out[s])


def _rows_are_the_scalar_ops(x, V, table, step, got):
    for r, rec in enumerate(_records(table)):
        assert int(got[r]) == _scalar(x, r, V, rec, step), (r, rec, step)


# ---------------------------------------------------------------------------------------- 1. ops.sample_rows_table --
def _recs(V):
    warp = dict(temperature=0.8, top_k=40, top_p=0.95, min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3)
    return [None,                                                         # six rows of random logits
            dict(top_k=5, seed=101, stream=3),
            dict(top_k=0, top_p=0.9, seed=102, stream=1),
            dict(warp, seed=2 ** 63 + 103, stream=7),
            dict(top_k=V + 5, seed=104, stream=2),
            dict(temperature=0.3, seed=105, stream=5),
            None,                                                         # a tie at the maximum
            dict(temperature=2.0, top_k=5, seed=106, stream=4),
            None,                                                         # NaN and -inf columns
            dict(top_p=0.9, seed=107, stream=6),
            None,                                                         # -inf only
            dict(warp, seed=108, stream=9)]


def _table_logits(V, ld, dtype, dev):
    x, _ = logits_host(V, 12, ld, 3.0, dtype)
    for r in (6, 7):
        x[r, 3] = x[r, V // 2] = x[r, V - 1] = 50.0
    for r in (8, 9):
        x[r, 0] = x[r, V - 2] = NAN
        x[r, 1] = x[r, V // 3] = x[r, V - 1] = NINF
    x[10:, :V] = NINF
    return x.to(dev)


@pytest.mark.parametrize("V,ld,dtype", [(V, ld, d) for V, ld in ((40, 48), (3077, 3077)) for d in ("bf16", "fp16", "fp32")]
                         + [(32007, 32064, "bf16")])
def test_every_row_of_a_table_launch_is_the_scalar_op_on_that_row(dev, V, ld, dtype):
    x = _table_logits(V, ld, dtype, dev)
    recs = _recs(V)
    assert len({r["seed"] for r in recs if r}) == len({r["stream"] for r in recs if r}) == 8      # all distinct
    table = ops.SampleTable(recs, dev)
    assert [u["mode"] for u in _records(table)] == [int(r is not None) for r in recs]
    perm = torch.tensor([5, 11, 0, 7, 3, 9, 1, 10, 2, 8, 6, 4], device=dev)
    for step in (0, 9):
        got = ops.sample_rows_table(x[:, :V], V, table, step)
        assert got.dtype == torch.long and int(got.min()) >= 0 and int(got.max()) < V             # never a pad column
        _rows_are_the_scalar_ops(x, V, table, step, got)
        # greedy rows: argmax_rows' tie, NaN and -inf behaviour; a sampled row without a finite logit emits the same
        am = ops.argmax_rows(x[:, :V], V)
        for r in (0, 6, 8, 10, 11):
            assert int(got[r]) == int(am[r]), r
        assert int(got[6]) == 3 and int(got[8]) == 0 and int(got[10]) == 0
        assert int(got[7]) in (3, V // 2, V - 1) and int(got[9]) not in (0, 1, V // 3, V - 2, V - 1)
        # position independence: permuting the rows of logits and table together permutes the ids
        ptab = ops.SampleTable([recs[i] for i in perm.tolist()], dev)
        assert torch.equal(ops.sample_rows_table(x[perm][:, :V], V, ptab, step), got[perm])
        assert torch.equal(ops.sample_rows_table(x[:, :V], V, table, step), got)                   # and it repeats
    # the seed, the stream and the step each reach the draw (row 5 at temperature 3: a wide distribution)
    if V > 1000:
        hot = dict(temperature=3.0, top_k=0, seed=1, stream=0)
        xs = x[5:6].expand(3, -1).contiguous()
        ids = torch.stack([ops.sample_rows_table(xs[:, :V], V, ops.SampleTable(
            [hot, dict(hot, seed=2), dict(hot, stream=1)], dev), s) for s in range(8)])
        assert not torch.equal(ids[:, 0], ids[:, 1]) and not torch.equal(ids[:, 0], ids[:, 2])
        assert len(set(ids[:, 0].tolist())) > 1


# --------------------------------------------------------------------------------- 2. ops.decode_emit_sample_table --
@pytest.mark.parametrize("dtype", ["bf16", "fp16", "fp32"])
def test_decode_emit_sample_table_keeps_decode_emits_books(dev, dtype):
    V, ld, pad, eos, B = 1000, 1008, 1003, 123, 3
    x, _ = logits_host(V, B, ld, 3.0, dtype, seed=3)
    x[0, eos] = 50.0                     # e^-40 of the mass elsewhere: top_p = 0.9 keeps this column alone
    x = x.to(dev)
    recs = [dict(top_k=0, top_p=0.9, seed=31, stream=2), None,
            dict(temperature=1.3, top_k=0, min_p=0.01, typical_p=0.95, seed=33, stream=1)]
    table = ops.SampleTable(recs, dev)
    col = 5
    tok = torch.full((B,), -1, dtype=torch.long, device=dev)
    done = torch.tensor([False, True, False], device=dev)
    out = torch.full((B, col + 4), -7, dtype=torch.long, device=dev)
    state = torch.tensor([11, col, 0, 0], dtype=torch.int32, device=dev)
    h_tok, h_done, h_out, h_state = tok.tolist(), done.tolist(), out.tolist(), state.tolist()
    select = lambda c: ops.sample_rows_table(x[:, :V], V, table, c).tolist()      # noqa: E731
    for call in range(2):
        ops.decode_emit_sample_table(x[:, :V], V, pad, eos, tok, done, out, state, table)
        R.emit(None, V, recs, pad, eos, h_tok, h_done, h_out, h_state, select=select)
        assert tok.tolist() == h_tok and done.tolist() == h_done and out.tolist() == h_out, call
        assert state.tolist() == h_state == [12 + call, col + 1 + call, 0, 0]
    assert h_out[0][col:col + 2] == [eos, pad] and h_out[1][col:col + 2] == [pad, pad] and h_done == [True, True, False]
    assert 0 <= h_out[2][col] < V and 0 <= h_out[2][col + 1] < V
    # refused calls return their codes and write nothing
    lib = L.load()
    before = [t.clone() for t in (tok, done, out, state)]
    ids = torch.full((B,), -9, dtype=torch.long, device=dev)

    def emit(table_p=table.records.data_ptr(), ld_=ld, dt=ops.dt(x)):
        return lib.mk_decode_emit_sample_table(x.data_ptr(), ld_, V, B, pad, eos, tok.data_ptr(), done.data_ptr(),
                                               out.data_ptr(), out.stride(0), state.data_ptr(), table_p, dt, None)

    def rows(table_p=table.records.data_ptr(), ld_=ld, dt=ops.dt(x)):
        return lib.mk_sample_rows_table(x.data_ptr(), ld_, B, V, table_p, 0, ids.data_ptr(), dt, None)

    for f in (emit, rows):
        assert f(table_p=None) == -1 and f(ld_=V - 1) == -1 and f(dt=7) == -2
    torch.cuda.synchronize()
    for a, b in zip(before, (tok, done, out, state)):
        assert torch.equal(a, b)
    assert ids.tolist() == [-9] * B
    with pytest.raises(L.MacawHipError, match="a SampleTable of 3 rows"):
        ops.sample_rows_table(x[:2, :V], V, table)
    with pytest.raises(L.MacawHipError, match="expected row-major"):
        ops.sample_rows_table(x.t()[:3], 3, table)
    with pytest.raises(L.MacawHipError, match="unsupported dtype"):
        ops.sample_rows_table(x[:, :V].double(), V, table)


# ---------------------------------------------------------------------------------------------- 3. generate() --
D1 = dict(temperature=0.9, top_k=20, top_p=0.9, seed=5)
D2 = dict(temperature=1.1, top_k=0, min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-3, seed=6)


def test_generate_one_request_is_the_scalar_call_bit_for_bit_on_every_path(dev):
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 1, dev)
    mask = torch.ones((1, 21), dtype=torch.long, device=dev)
    mask[0, :4] = 0
    for path in (dict(), dict(decode_graph=False), dict(use_cache=False), dict(attention_mask=mask),
                 dict(attention_mask=mask, decode_graph=False)):
        for d in (D1, D2):
            got = lm.generate(sampling_params=[d], **kw, **path)
            assert got.shape == (1, 12) and torch.equal(got, lm.generate(do_sample=True, **d, **kw, **path)), (path, d)
    # seed=None: the scalar call's one draw from torch's generator
    free = {k: v for k, v in D1.items() if k != "seed"}
    torch.manual_seed(123)
    a = lm.generate(sampling_params=[free], **kw)
    torch.manual_seed(123)
    assert torch.equal(a, lm.generate(do_sample=True, **free, **kw))
    # num_samples: row j is stream j, the scalar call's row index
    for path in (dict(), dict(decode_graph=False), dict(use_cache=False)):
        for d in (D1, D2):
            got = lm.generate(sampling_params=[d], num_samples=4, **kw, **path)
            want = lm.generate(do_sample=True, num_samples=4, **d, **kw, **path)
            assert got.shape == (4, 12) and torch.equal(got, want), (path, d)
    assert len({tuple(r) for r in got.tolist()}) > 1                      # the streams differ


class _Capture:
    """wraps ops.sample_rows_table: records every call's logits (cloned), table and step"""

    def __enter__(self):
        self.steps, self.real = [], ops.sample_rows_table

        def wrapped(x, cols, table, step=0):
            self.steps.append((x.clone(), cols, table, step))
            return self.real(x, cols, table, step)
        ops.sample_rows_table = wrapped
        return self

    def __exit__(self, *exc):
        ops.sample_rows_table = self.real


def test_generate_mixed_batch_selects_every_row_by_its_own_record(dev):
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    kw = _kw(cfg_l, 3, dev)
    hot = dict(temperature=3.0, top_k=0, seed=21)                         # a wide distribution: another seed must show
    sp = [None, hot, D2]
    with _Capture() as cap, _Spy("argmax_rows", "sample_rows", "sample_rows_warp", "decode_emit_sample_table") as spy:
        e = lm.generate(sampling_params=sp, decode_graph=False, **kw)
        assert len(cap.steps) == 12 and [s[3] for s in cap.steps] == list(range(12))
        assert spy.calls["argmax_rows"] == spy.calls["sample_rows"] == spy.calls["sample_rows_warp"] == []
        assert spy.calls["decode_emit_sample_table"] == []
    assert e.shape == (3, 12)
    recs = _records(cap.steps[0][2])
    assert [r["mode"] for r in recs] == [0, 1, 1] and [r["stream"] for r in recs] == [0, 0, 0]
    assert [r["seed"] for r in recs[1:]] == [21, 6]
    for x, cols, table, step in cap.steps:
        assert cols == V and table is cap.steps[0][2]                     # built once per call
        x2 = x if x.dim() == 2 and x.stride(1) == 1 else x.contiguous()
        _rows_are_the_scalar_ops(x2, V, table, step, e[:, step])
        assert int(e[0, step]) == int(ops.argmax_rows(x2[:, :V], V)[0])   # the greedy row of every step
    with _Spy("decode_emit_sample_table", "sample_rows_table", "decode_emit", "decode_emit_sample") as spy:
        g = lm.generate(sampling_params=sp, **kw)                         # the graph path: token 0, one eager step, a capture
        assert len(spy.calls["decode_emit_sample_table"]) == 3 and spy.calls["sample_rows_table"] == []
        assert spy.calls["decode_emit"] == spy.calls["decode_emit_sample"] == []
    assert torch.equal(g, e)
    assert torch.equal(lm.generate(sampling_params=sp, **kw), g)          # the same call twice
    other = lm.generate(sampling_params=[None, dict(hot, seed=22), D2], **kw)
    assert not torch.equal(other[1], g[1])                                # another seed: row 1 changes ...
    assert torch.equal(other[0], g[0]) and torch.equal(other[2], g[2])    # ... and it alone
    one = dict(_kw(cfg_l, 3, dev), input_ids=kw["input_ids"][1:2])
    assert not torch.equal(lm.generate(do_sample=True, **hot, **one),     # the scalar call shows the change too
                           lm.generate(do_sample=True, **dict(hot, seed=22), **one))
    # temperature == 0 is the greedy row
    assert torch.equal(lm.generate(sampling_params=[dict(temperature=0, seed=1), hot, D2], **kw), g)


def test_generate_compositions_equal_their_eager_twins(dev):
    from macaw_llm_amd.grammar import TokenDFA
    lm, cfg_l = _small_llama(dev)
    V = cfg_l["vocab_size"]
    kw = _kw(cfg_l, 3, dev)
    sp = [D1, None, D2]
    even = TokenDFA.from_edges(1, [(0, t, 0) for t in range(0, V, 2)], [0], vocab_size=V)
    on = dict(grammar=[even, None, even], logit_bias=[{4: 3.0}, {7: 100.0}, None], return_logprobs=True)
    a = lm.generate(sampling_params=sp, **on, **kw)
    b = lm.generate(sampling_params=sp, decode_graph=False, **on, **kw)
    assert torch.equal(a.ids, b.ids) and a.ids.shape == (3, 12)
    assert bool((a.ids[0] % 2 == 0).all()) and bool((a.ids[2] % 2 == 0).all()) and bool((a.ids[1] == 7).all())
    assert bool(torch.isfinite(a.logprobs).all()) and bool(torch.isfinite(b.logprobs).all())
    assert float(a.logprobs[1].abs().max()) <= 1e-6                       # +100: the other columns hold e^-80 of the mass
    neg = dict(guidance_scale=1.5, negative_prompt_ids=_ids(cfg_l, 3, dev, S=5))
    assert torch.equal(lm.generate(sampling_params=sp, **neg, **kw),
                       lm.generate(sampling_params=sp, decode_graph=False, **neg, **kw))
    # decode_weights="fp8" runs on the hipGraph path alone (generate refuses decode_graph=False next to it), so it has no
    # eager twin: its twins are the scalar calls, bit for bit -- one request, and one request's n streams -- and in the
    # mixed batch the greedy row is the greedy call's row
    w8 = dict(decode_weights="fp8")
    with pytest.raises(ValueError, match="decode_weights='fp8'"):
        lm.generate(sampling_params=sp, decode_graph=False, **w8, **kw)
    k1 = _kw(cfg_l, 1, dev)
    for d in (D1, D2):
        assert torch.equal(lm.generate(sampling_params=[d], **w8, **k1), lm.generate(do_sample=True, **d, **w8, **k1))
        assert torch.equal(lm.generate(sampling_params=[d], num_samples=3, **w8, **k1),
                           lm.generate(do_sample=True, num_samples=3, **d, **w8, **k1))
    m8 = lm.generate(sampling_params=sp, **w8, **kw)
    assert torch.equal(m8, lm.generate(sampling_params=sp, **w8, **kw)) and torch.equal(m8[1], lm.generate(**w8, **kw)[1])
    # a session's second turn
    turn = dict(eos_token_id=-1, pad_token_id=0, max_new_tokens=8, sampling_params=sp)
    nxt = _ids(cfg_l, 3, dev, S=4)
    _, s1 = lm.generate(input_ids=kw["input_ids"], return_session=True, **turn)
    _, s2 = lm.generate(input_ids=kw["input_ids"], return_session=True, **turn)
    two = lm.generate(input_ids=nxt, session=s1, **turn)
    assert two.shape == (3, 8) and torch.equal(two, lm.generate(input_ids=nxt, session=s2, decode_graph=False, **turn))


def test_all_greedy_lists_and_the_default_call_none_of_the_new_ops(dev):
    lm, cfg_l = _small_llama(dev)
    kw = _kw(cfg_l, 2, dev)
    with _Spy("sample_rows_table", "decode_emit_sample_table") as spy:
        real, built = ops.SampleTable, []

        class Counting(real):
            def __init__(self, *a, **k):
                built.append(a)
                super().__init__(*a, **k)
        ops.SampleTable = Counting
        try:
            for path in (dict(), dict(decode_graph=False), dict(use_cache=False)):
                greedy = lm.generate(**kw, **path)
                for off in (None, [None, None], [dict(temperature=0), None], (dict(temperature=0.0, top_k=3), None)):
                    assert torch.equal(lm.generate(sampling_params=off, **kw, **path), greedy), (path, off)
            lm.generate(num_beams=2, sampling_params=None, **kw)
        finally:
            ops.SampleTable = real
        assert spy.calls["sample_rows_table"] == spy.calls["decode_emit_sample_table"] == built == []
    # the refusals that need the real batch
    with pytest.raises(ValueError, match="sampling_params holds 3 entries for 2 prompts"):
        lm.generate(sampling_params=[None, D1, D2], **kw)
    with pytest.raises(ValueError, match=r"sampling_params\[1\]: top_p must lie in \(0, 1\], got 1.5"):
        lm.generate(sampling_params=[None, dict(top_p=1.5)], **kw)
    with pytest.raises(ValueError, match="num_beams=2.*not built"):
        lm.generate(sampling_params=[None, D1], num_beams=2, **kw)


def test_set_sampling_params_reaches_the_loop(dev):
    from test_model_gpu import build_model, to_dev
    fx = load_case("micro_all")
    model = build_model(configs.get(fx["config_name"]), fx["state"], torch.bfloat16, dev, fuse=True).eval()
    inp = to_dev(fx["inputs"], dev)
    inp["inference"] = True
    B = inp["input_ids"].shape[0]
    with torch.no_grad(), _Spy("decode_emit", "decode_emit_sample_table") as spy:
        base = model(inputs=inp)
        assert spy.calls["decode_emit_sample_table"] == [] and len(spy.calls["decode_emit"]) > 0
        Mo.MM_LLMs.set_sampling_params([dict(temperature=0.9, top_k=30, seed=4 + b) for b in range(B)])
        ids = model(inputs=inp)
        calls = spy.calls["decode_emit_sample_table"]
        recs = _records(calls[0][8])
        assert len(calls) > 0 and [(r["mode"], r["top_k"], r["seed"], r["stream"]) for r in recs] == \
            [(1, 30, 4 + b, 0) for b in range(B)]
        assert torch.equal(ids, model(inputs=inp))                        # integer seeds: the same ids again
        Mo.MM_LLMs.set_sampling_params([dict(temperature=0)] * B)
        n = len(calls)
        assert torch.equal(model(inputs=inp), base) and len(spy.calls["decode_emit_sample_table"]) == n
        Mo.MM_LLMs.set_sampling_params()
        assert torch.equal(model(inputs=inp), base) and len(spy.calls["decode_emit_sample_table"]) == n
    assert ids.dtype == torch.long and ids.shape[0] == base.shape[0]
