"""CPU: frequency_penalty, presence_penalty and logit_bias of generate() -- the rule of include/macaw_hip.h, "Per-request
penalties", as restated in tests/penalties_ref.py against an independent formulation and against vLLM's formula written
out here, the header, the ctypes prototype and the exported symbol's error codes, ops.BiasTable, the public arguments,
MM_LLMs.set_penalties and every refusal."""
import inspect
import os
import re

import pytest
import torch

import penalties_ref as R

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
INF, NAN = float("inf"), float("nan")
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _same(a, b):
    return a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------- 1. the reference vs the independent formulation --
def test_reference_equals_the_dense_fp64_formulation_on_random_integer_rows():
    """integer-valued logits in [-40, 40], f and p in {-2 .. 2}, biases in [-100, 100], counts <= 24: every intermediate
    is an integer of magnitude <= 40 + 100 + 2 * 24 + 2 = 190 < 2^8, exact in fp32 and in fp64, so the two formulations
    hand the same exact number to the one final rounding"""
    g = torch.Generator().manual_seed(0)
    for case in range(60):
        B, V = int(torch.randint(1, 4, (1,), generator=g)), int(torch.randint(1, 70, (1,), generator=g))
        ld, n_max = V + int(torch.randint(0, 5, (1,), generator=g)), int(torch.randint(1, 25, (1,), generator=g))
        dtype = DTYPES[case % 3]
        logits = torch.randint(-40, 41, (B, ld), generator=g).to(dtype)
        gen = torch.randint(-2, V + 2, (B, n_max), generator=g)
        n = int(torch.randint(0, n_max + 1, (1,), generator=g))
        f = torch.randint(-2, 3, (B,), generator=g).tolist() if case % 4 else None
        p = torch.randint(-2, 3, (B,), generator=g).tolist() if case % 5 else None
        bias = None
        if case % 2:
            bias = [None if b == 1 else {int(c): float(torch.randint(-100, 101, (1,), generator=g))
                                         for c in torch.randperm(V, generator=g)[:int(torch.randint(0, V + 1, (1,), generator=g))]}
                    for b in range(B)]
        want, dense = R.penalize(logits, V, gen, n, f, p, bias), R.penalize_dense(logits, V, gen, n, f, p, bias)
        assert _same(want, dense), case
        assert _same(want[:, V:], logits[:, V:])


def test_reference_on_hand_written_rows():
    V = 6
    x = torch.tensor([[1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 9.0]])                          # ld = 7: one padding column
    gen = torch.tensor([[2, 2, 2, 2, 0]])
    # a repeated id (count = n)
    assert R.penalize(x, V, gen, 4, [0.5], [0.25]).tolist() == [[1.0, 2.0, 3.0 - 2.0 - 0.25, 4.0, 5.0, 6.0, 9.0]]
    assert R.penalize(x, V, gen, 5, [0.5], [0.25]).tolist() == [[1.0 - 0.5 - 0.25, 2.0, 0.75, 4.0, 5.0, 6.0, 9.0]]
    # n = 0: only the bias; n beyond n_max is clamped
    assert R.penalize(x, V, gen, 0, [2.0], [2.0], [{5: -1.5}]).tolist() == [[1.0, 2.0, 3.0, 4.0, 5.0, 4.5, 9.0]]
    assert _same(R.penalize(x, V, gen, 99, [0.5], [0.25]), R.penalize(x, V, gen, 5, [0.5], [0.25]))
    # an id outside [0, V) names no column (6 is the padding column, -1 nothing)
    out = torch.tensor([[6, -1, 7, 1 << 40]])
    assert _same(R.penalize(x, V, out, 4, [1.0], [1.0]), x)
    # bias and count on one column: (x + beta) - f * cnt - p, one result; negative penalties raise the logit
    assert R.penalize(x, V, gen, 4, [1.0], [0.5], [{2: 10.0, 1: 1.0}]).tolist() == [[1.0, 3.0, 3.0 + 10 - 4 - 0.5, 4.0, 5.0, 6.0, 9.0]]
    assert R.penalize(x, V, gen, 4, [-1.0], [-0.5]).tolist() == [[1.0, 2.0, 3.0 + 4 + 0.5, 4.0, 5.0, 6.0, 9.0]]
    # f = p = 0: a generated column is NOT touched; presence alone, frequency alone
    assert _same(R.penalize(x, V, gen, 5, [0.0], [0.0]), x) and _same(R.penalize(x, V, gen, 5), x)
    assert R.penalize(x, V, gen, 5, None, [1.0]).tolist() == [[0.0, 2.0, 2.0, 4.0, 5.0, 6.0, 9.0]]
    assert R.penalize(x, V, gen, 5, [1.0], None).tolist() == [[0.0, 2.0, -1.0, 4.0, 5.0, 6.0, 9.0]]
    for fn in (R.penalize, R.penalize_dense):
        # -inf / NaN / +inf columns stay what they are, touched by a count, a bias or both
        s = torch.tensor([[-INF, NAN, INF, -INF, NAN, INF, 0.0]])
        got = fn(s, V, torch.tensor([[0, 1, 2, 2]]), 4, [-2.0], [2.0], [{2: -100.0, 3: 100.0, 4: 1.0, 5: -100.0}])
        assert got[0, [0, 3]].tolist() == [-INF, -INF] and got[0, [2, 5]].tolist() == [INF, INF]
        assert bool(got[0, [1, 4]].isnan().all()) and got[0, 6] == 0.0
    # untouched columns keep their bits: -0.0 and a NaN payload
    for dtype in DTYPES:
        s = torch.tensor([[-0.0, 1.0, NAN, 2.0]]).to(dtype)
        _bits(s)[0, 2] |= 5                                                          # a payload in the mantissa's low bits
        got = R.penalize(s, 4, torch.tensor([[1]]), 1, [1.0], [1.0], [{3: 1.0}])
        assert _same(got[:, [0, 2]], s[:, [0, 2]]) and got[0, 1] == -1.0 and got[0, 3] == 3.0
        assert _same(R.penalize_dense(s, 4, torch.tensor([[1]]), 1, [1.0], [1.0], [{3: 1.0}]), got)


def test_every_operation_is_rounded_by_itself_and_the_result_once():
    """values at which a fused multiply-add, another order or a second rounding would show"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32)
    x, f, cnt, p, beta = 0.1, 0.3, 7, 0.7, 33.3
    want = ((f32(x) + f32(beta)) - f32(f) * f32(float(cnt))) - f32(p)
    got = R.penalize(f32([[x]]), 1, torch.zeros((1, cnt), dtype=torch.long), cnt, [f], [p], [{0: beta}])
    assert _same(got, want.reshape(1, 1))
    # bf16: 256 + 1 rounds to 256 (a tie to even) and 256 - 1 = 255 is exact in 8 bits: bias and count together give 256
    # + 1 - 1 = 256 with ONE rounding; rounding behind the bias and again behind the count would give 256 -> 255
    b = torch.tensor([[256.0]], dtype=torch.bfloat16)
    got = R.penalize(b, 1, torch.zeros((1, 1), dtype=torch.long), 1, [1.0], [0.0], [{0: 1.0}])
    assert got.tolist() == [[256.0]]
    assert (b + 1.0 - 1.0).tolist() == [[255.0]]                                     # what two roundings would give


# ------------------------------------------------------------------------------------------ 2. vLLM's formula --
def _vllm(logits, V, gen, n, f, p, bias):
    """vLLM's sampler on fp32 rows: logit_bias is added first, then apply_penalties' two lines for the OpenAI penalties
    (output tokens only): logits -= frequency_penalties * output_bin_counts; logits -= presence_penalties *
    output_mask.  Written out here; nothing is imported from vLLM"""
    B = logits.shape[0]
    lg = logits[:, :V].clone()
    for b in range(B):
        for c, v in ((bias[b] if bias else None) or {}).items():
            lg[b, c] += v
    counts = torch.zeros((B, V + 1), dtype=torch.long)
    ids = gen[:, :n].clone()
    ids[(ids < 0) | (ids >= V)] = V                                                  # vLLM's padding bin
    counts.scatter_add_(1, ids, torch.ones_like(ids))
    counts = counts[:, :V]
    mask = counts > 0
    lg -= torch.tensor(f, dtype=torch.float32).unsqueeze(1) * counts
    lg -= torch.tensor(p, dtype=torch.float32).unsqueeze(1) * mask
    return lg


def test_reference_equals_vllms_formula_on_finite_rows():
    g = torch.Generator().manual_seed(1)
    for case in range(40):
        B, V, n_max = 3, int(torch.randint(2, 60, (1,), generator=g)), 30
        logits = torch.randn((B, V + 3), generator=g) * 8
        gen = torch.randint(0, V, (B, n_max), generator=g) % max(1, V // 3)           # many repeats
        n = int(torch.randint(0, n_max + 1, (1,), generator=g))
        f = ((torch.rand(B, generator=g) * 4 - 2) * (torch.rand(B, generator=g) < 0.8)).tolist()
        p = ((torch.rand(B, generator=g) * 4 - 2) * (torch.rand(B, generator=g) < 0.8)).tolist()
        bias = [{int(c): float(torch.rand(1, generator=g) * 200 - 100) for c in torch.randperm(V, generator=g)[:V // 2]}
                if b != case % 3 else None for b in range(B)]
        want = R.penalize(logits, V, gen, n, f, p, bias)
        assert torch.equal(want[:, :V], _vllm(logits, V, gen, n, f, p, bias)), case
        assert _same(want[:, V:], logits[:, V:])


# ---------------------------------------------------------------------------------------------------- the ABI --
def test_header_declares_the_entry_point_with_the_prototypes_arity_and_states_the_rule():
    src = open(HEADER).read()
    m = re.search(r"^int mk_logits_penalize\((.*?)\);", src, flags=re.M | re.S)
    assert m, "mk_logits_penalize is not declared in include/macaw_hip.h"
    assert len(m.group(1).split(",")) == len(L.SIGNATURES["mk_logits_penalize"]) == 16
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION
    for phrase in ("the GENERATED ids only", "The prompt is never counted", "x = x - (f_b * float(cnt_c));  x = x - p_b",
                   "no fused multiply-add", "-inf stays -inf and a NaN stays NaN", "+inf stays +inf",
                   "keep their bits exactly", "Token 0 (n = 0) sees only the bias", "n_max <= 2^24",
                   "BEHIND mk_logits_process and in front of mk_seq_ban", "vLLM adds logit_bias in front of repetition_penalty",
                   "nothing is launched", "V <= 2^18 = 262144"):
        assert phrase in src, phrase
    assert src.index("int mk_logits_process(") < src.index("int mk_logits_penalize(") < src.index("int mk_seq_ban(")
    assert "penalty.hip" in __import__("macaw_llm_amd.build", fromlist=["SOURCES"]).SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "penalty.hip")).read()
    assert "asm" not in kernel and "fmaf" not in kernel                  # plain loads and stores, LDS atomics, no fma
    assert "contract(off)" in kernel


def test_the_compiled_kernel_holds_no_fused_multiply_add(tmp_path):
    """hipcc contracts a * b - c by default; the rule rounds f * count by itself.  The kernel's only fp32 arithmetic is
    the rule, so its gfx950 assembly must hold a multiply and subtractions and no fma / mad / fmac"""
    import subprocess
    from macaw_llm_amd import build
    out = tmp_path / "penalty.s"
    subprocess.check_call([build._hipcc(), *build.FLAGS, *build.FILE_FLAGS.get("penalty.hip", []), "-S", "--cuda-device-only",
                           "-o", str(out), os.path.join(ROOT, "macaw_llm_amd", "csrc", "penalty.hip")],
                          stderr=subprocess.DEVNULL)
    asm = out.read_text()
    assert asm.count("logits_penalize_kernel") >= 3
    assert not re.search(r"\bv_(fma|mad|fmac)\w*_f32", asm)
    assert len(re.findall(r"\bv_mul_f32", asm)) >= 3 and len(re.findall(r"\bv_sub_f32", asm)) >= 3


def test_the_library_exports_it_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    fn = lib.mk_logits_penalize
    sig = L.SIGNATURES["mk_logits_penalize"]
    assert fn(*[None if t is L._vp else t(0) for t in sig]) == -1      # null pointers: a code, nothing launched
    fake = 4096                                                         # never dereferenced: every call below is refused

    def call(logits=fake, ld=64, V=64, B=1, out=fake, out_ld=8, n_max=8, n_dev=None, n_add=0, f=fake, p=fake, off=None,
             ids=None, val=None, dtype=L.MK_F32):
        return fn(logits, ld, V, B, out, out_ld, n_max, n_dev, n_add, f, p, off, ids, val, dtype, None)

    for bad in (dict(logits=None), dict(out=None), dict(B=0), dict(B=-1), dict(V=0), dict(ld=63), dict(n_max=-1),
                dict(n_max=(1 << 24) + 1, out_ld=1 << 25), dict(out_ld=7), dict(off=fake), dict(off=fake, ids=fake),
                dict(off=fake, val=fake)):
        assert call(**bad) == -1, bad
    assert call(V=(1 << 18) + 1, ld=(1 << 18) + 1) == -2               # the bitmap's LDS budget
    assert call(dtype=L.MK_FP8) == -2
    # f, p and bias_off all null: success without a launch (the pointers are not device memory)
    assert call(f=None, p=None) == 0 and call(f=None, p=None, ids=fake, val=fake, n_max=1 << 24, out_ld=1 << 24) == 0
    assert "mk_logits_penalize" in inspect.getsource(ops.logits_penalize)


# ---------------------------------------------------------------------------------------------- 4. BiasTable --
def test_bias_table_builds_sorted_distinct_in_range_csr_arrays():
    t = ops.BiasTable([{7: 1.5, 2: -3.0, 5: 100}, None, {}, {0: -100.0}], 4, 8, "cpu")
    assert t.on and t.B == 4
    assert (t.off.dtype, t.ids.dtype, t.val.dtype) == (torch.int32, torch.int32, torch.float32)
    assert t.off.tolist() == [0, 3, 3, 3, 4] and t.ids.tolist() == [2, 5, 7, 0] and t.val.tolist() == [-3.0, 100.0, 1.5, -100.0]
    one = ops.BiasTable({3: 1.0, 1: 2.0}, 3, 4, "cpu")                  # one dict: every row
    assert one.off.tolist() == [0, 2, 4, 6] and one.ids.tolist() == [1, 3] * 3 and one.val.tolist() == [2.0, 1.0] * 3
    g = torch.Generator().manual_seed(2)
    rows = [{int(c): float(i) for i, c in enumerate(torch.randperm(5000, generator=g)[:k])} for k in (1024, 0, 17)]
    big = ops.BiasTable(rows, 3, 5000, "cpu")
    off, ids = big.off.tolist(), big.ids.tolist()
    assert off == [0, 1024, 1024, 1041]
    for b in range(3):
        r = ids[off[b]:off[b + 1]]
        assert r == sorted(set(r)) and all(0 <= c < 5000 for c in r)
        assert {c: v for c, v in zip(r, big.val.tolist()[off[b]:off[b + 1]])} == rows[b]
    for off_rows in (None, [None, None], [None, {}], [{}, {}]):         # no entry anywhere: off, nothing allocated
        t = ops.BiasTable(off_rows, 2, 8, "cpu")
        assert not t.on and t.off is None and t.ids is None and t.val is None and t.B == 2
    for bad in ([{8: 1.0}], [{-1: 1.0}], [{1.5: 1.0}], [{True: 1.0}], [{1: NAN}], [{1: INF}], [{1: "2"}], [[1, 2]],
                [{1: 1.0}, None], [{c: 0.5 for c in range(1025)}]):
        with pytest.raises(L.MacawHipError, match="BiasTable"):
            ops.BiasTable(bad, 1, 8 if len(bad[0]) < 1000 else 4096, "cpu")
    assert ops.MAX_BIAS == Mo.MAX_LOGIT_BIAS == 1024


# ------------------------------------------------------------------------------ 3. public arguments and refusals --
def test_generate_and_set_penalties_carry_the_new_arguments():
    want = dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None)
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for k, v in want.items():
        assert p[k].default == v and type(p[k].default) is type(v), k
    p = inspect.signature(Mo.MM_LLMs.set_penalties).parameters
    assert {k: p[k].default for k in p} == want
    assert Mo.PENALTIES[0] == want
    try:
        Mo.MM_LLMs.set_penalties(frequency_penalty=0.5, presence_penalty=[0.1, -0.2], logit_bias={3: 5})
        assert Mo.PENALTIES[0] == dict(frequency_penalty=0.5, presence_penalty=[0.1, -0.2], logit_bias={3: 5})
        with pytest.raises(ValueError, match="frequency_penalty"):
            Mo.MM_LLMs.set_penalties(frequency_penalty=2.5)
        assert Mo.PENALTIES[0]["frequency_penalty"] == 0.5              # a refused call changes nothing
        Mo.MM_LLMs.set_penalties(presence_penalty=torch.tensor([1.0, 0.0]))
        assert Mo.PENALTIES[0] == dict(frequency_penalty=0.0, presence_penalty=[1.0, 0.0], logit_bias=None)
    finally:
        Mo.MM_LLMs.set_penalties()
    assert Mo.PENALTIES[0] == want
    fwd = inspect.getsource(Mo.MM_LLMs.forward)
    assert "PENALTIES[0] != _PENALTIES_OFF" in fwd and "par.update(PENALTIES[0])" in fwd
    doc = Mo.LlamaForCausalLM.generate.__doc__
    for phrase in ("frequency_penalty, presence_penalty, logit_bias", "the count restarts with every call"):
        assert phrase in doc, phrase


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(B=1, **kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(B, 2, 4, dtype=torch.bfloat16), **kw)


def test_every_refusal_is_a_value_error_before_the_model_is_touched():
    for name in ("frequency_penalty", "presence_penalty"):
        # range violations, and what is no number
        for bad in (2.5, -2.0001, NAN, INF, -INF, "0.5", None, True, [0.5, 3.0], torch.tensor([0.0, NAN]), [[0.5, 0.5]],
                    torch.zeros(2, 1)):
            with pytest.raises(ValueError, match=name):
                _generate(B=2, **{name: bad})
            with pytest.raises(ValueError, match=name):
                Mo.MM_LLMs.set_penalties(**{name: bad})
        # wrong counts
        for bad in ([0.5], [0.5, 0.5, 0.5], torch.tensor([0.5]), (), torch.zeros(0)):
            with pytest.raises(ValueError, match=rf"{name} holds {len(bad)} values for 2 prompts"):
                _generate(B=2, **{name: bad})
        for ok in (2, -2.0, 0.5, [0.5, 0.0], (0.0, 0.0), torch.tensor([1.0, -1.0]), torch.tensor(0.25)):
            with pytest.raises(_PastTheChecks):
                _generate(B=2, **{name: ok})
    # logit_bias: a bad id, a bad value, too many entries, a non-dict, a wrong count
    for bad in ({-1: 1.0}, {1.0: 1.0}, {"3": 1.0}, {True: 1.0}, {3: 100.5}, {3: -101}, {3: NAN}, {3: INF}, {3: "1"},
                {3: None}, {3: True}, {c: 1.0 for c in range(1025)}, [(3, 1.0)], "3", 5, [{3: 1.0}, [3]], [{3: 1.0}, 7],
                [None, {-2: 1.0}]):
        with pytest.raises(ValueError, match="logit_bias"):
            _generate(B=2, logit_bias=bad)
        with pytest.raises(ValueError, match="logit_bias"):
            Mo.MM_LLMs.set_penalties(logit_bias=bad)
    for bad in ([{3: 1.0}], [None, None, {3: 1.0}], []):
        with pytest.raises(ValueError, match=rf"logit_bias holds {len(bad)} entries for 2 prompts"):
            _generate(B=2, logit_bias=bad)
    for ok in ({3: 100, 0: -100.0}, {c: 1.0 for c in range(1024)}, [None, {3: 1.0}], [None, None], {}, [{}, {}]):
        with pytest.raises(_PastTheChecks):
            _generate(B=2, logit_bias=ok)
    assert Mo.PENALTIES[0] == dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None)
    # what it does not compose with
    for on in (dict(frequency_penalty=0.5), dict(presence_penalty=-1.0), dict(logit_bias={3: 1.0}),
               dict(frequency_penalty=[0.0, 0.1])):
        with pytest.raises(ValueError, match=r"frequency_penalty=, presence_penalty=, logit_bias=.*num_beams=2.*not built"):
            _generate(B=2, num_beams=2, **on)
        with pytest.raises(ValueError, match=r"frequency_penalty=, presence_penalty=, logit_bias=.*prompt_lookup_num_tokens=4"
                                             r".*not built"):
            _generate(B=2, prompt_lookup_num_tokens=4, **on)
        with pytest.raises(_PastTheChecks):
            _generate(B=2, **on)
    # everything off, in every spelling: untouched by the refusals
    for off in (dict(), dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None), dict(frequency_penalty=0),
                dict(presence_penalty=[0.0, 0.0]), dict(logit_bias=[None, {}])):
        for other in (dict(num_beams=2), dict(prompt_lookup_num_tokens=4)):
            with pytest.raises(_PastTheChecks):
                _generate(B=2, **off, **other)
    assert Mo._penalties_check("generate", 0.0, 0, None, 2) is None
    assert Mo._penalties_check("generate", 0.5, 0.0, {1: 2}, 2) == ([0.5, 0.5], None, [{1: 2}, {1: 2}])
    assert Mo._penalties_check("generate", [0, 0], (0.0, 1), [None, {4: 1.0}], 2) == (None, [0.0, 1.0], [None, {4: 1.0}])


def test_an_id_beyond_the_vocabulary_is_refused_once_the_model_is_known_and_before_any_launch(monkeypatch):
    from transformers import LlamaConfig
    lm = Mo.LlamaForCausalLM(LlamaConfig(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=2, vocab_size=40, max_position_embeddings=64)).to(torch.bfloat16)
    monkeypatch.setattr(Mo, "_dev_check", lambda t: None)
    launched = []
    monkeypatch.setattr(L, "load", lambda: launched.append(1) or (_ for _ in ()).throw(_PastTheChecks("the library")))
    x = torch.zeros(2, 3, 32, dtype=torch.bfloat16)
    for bad in ({40: 1.0}, [None, {39: 1.0, 1 << 20: 1.0}]):
        with pytest.raises(ValueError, match=r"logit_bias: token id \d+ is not an integer in \[0, 40\)"):
            lm.generate(inputs_embeds=x, max_new_tokens=4, logit_bias=bad)
    assert not launched
    with pytest.raises(_PastTheChecks):                                 # 39 is inside: on to the device
        lm.generate(inputs_embeds=x, max_new_tokens=4, logit_bias={39: 1.0})
    assert launched


# ------------------------------------------------------------------------------- the defaults launch nothing --
def test_the_defaults_record_the_plain_calls_launches_and_the_launch_sits_between_the_processors_and_the_emit(monkeypatch):
    """the recorders of tests/test_generate_trace_cpu.py: generate() on CPU tensors, every launch logged.  With the
    defaults spelled out the log is the plain call's, entry for entry, and ops.logits_penalize is never reached; with a
    penalty on it is reached once per eager emit, behind logits_process and in front of the emit, with n_dev = state + 1
    in the graph loop and the host's count in the eager loop"""
    import test_generate_trace_cpu as T
    off = dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None)
    seen = []
    for mode in (dict(), dict(kw=dict(decode_graph=False)), dict(kw=dict(use_cache=False)), dict(kw=dict(T.PROC))):
        logs = []
        for extra in ({}, off):
            with monkeypatch.context() as mp:
                mp.setattr(ops, "logits_penalize", lambda *a, **k: seen.append(a))
                spec = dict(mode, N=6, kw=dict(mode.get("kw", {}), **extra))
                tr, res = T.call(mp, spec)
                logs.append((tr.log, res))
        assert logs[0] == logs[1] and isinstance(logs[0][1], list)
        assert not any("penal" in str(e[0]) for e in logs[0][0] if isinstance(e, list))
    assert seen == []
    for mode, n_calls in ((dict(), 3), (dict(kw=dict(decode_graph=False)), 6), (dict(kw=dict(use_cache=False)), 6)):
        with monkeypatch.context() as mp:
            order = []
            tr, res = None, None

            def penalize(lg, V, gen, n_dev=None, n_add=0, frequency=None, presence=None, bias=None):
                order.append(("penalize", n_dev is not None, n_add, frequency.tolist(), presence, bias.ids.tolist()))
                return lg
            mp.setattr(ops, "logits_penalize", penalize)
            spec = dict(mode, N=6, kw=dict(mode.get("kw", {}), **T.PROC, frequency_penalty=[0.5, 0.0], logit_bias={7: 1.0}))
            real = T.GenTrace._rec

            def rec(self, name, sig, eff):
                inner = real(self, name, sig, eff)
                if name not in ("logits_process", "decode_emit", "argmax_rows"):
                    return inner

                def outer(*a, **k):
                    order.append((name,))
                    return inner(*a, **k)
                return outer
            mp.setattr(T.GenTrace, "_rec", rec)
            tr, res = T.call(mp, spec)
        assert isinstance(res, list), res
        pens = [e for e in order if e[0] == "penalize"]
        assert len(pens) == n_calls, (mode, order)
        graph = not mode
        for i, e in enumerate(pens):
            assert e[3] == [0.5, 0.0] and e[4] is None and e[5] == [7, 7]
            assert e[1] == graph and (graph or e[2] == i)             # state + 1 on the device / the host's count
        names = [e[0] for e in order]
        for i, n in enumerate(names):                                  # processors -> penalties -> the selection
            if n == "penalize":
                assert names[i - 1] == "logits_process" and names[i + 1] in ("decode_emit", "argmax_rows"), names
