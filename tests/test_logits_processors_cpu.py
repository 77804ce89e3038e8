"""CPU: the logits processors of generate() -- the rule of include/macaw_hip.h as restated in tests/logits_proc_ref.py
against the installed transformers' three processors chained in HF's order (fp32, bit for bit), the restatement's
rounding for 16-bit logits, the header and the ctypes prototype, the exported symbol and its error codes, the public
arguments, MM_LLMs.set_logits_processors and every refusal."""
import inspect
import os
import re

import pytest
import torch

import logits_proc_ref as R

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
INF = float("inf")


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _hf(logits, prompt, generated, theta, n, m, eos):
    """the installed processors in the order HF's generate() chains them: repetition penalty, n-gram, min new tokens"""
    from transformers.generation.logits_process import (MinNewTokensLengthLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor)
    ids = torch.tensor([list(prompt) + list(generated)], dtype=torch.long)
    s = logits[None].clone()
    if theta != 1.0:
        s = RepetitionPenaltyLogitsProcessor(penalty=float(theta))(ids, s)
    if n > 0:
        s = NoRepeatNGramLogitsProcessor(n)(ids, s)
    s = MinNewTokensLengthLogitsProcessor(len(prompt), m, eos)(ids, s)
    return s[0]


def _history(g, V, L_, dup):
    """L_ ids; dup: drawn from 5 values only, so that ids and n-grams repeat"""
    if dup:
        pool = torch.randint(0, V, (5,), generator=g)
        return pool[torch.randint(0, 5, (L_,), generator=g)].tolist()
    return torch.randint(0, V, (L_,), generator=g).tolist()


def _logits(g, V):
    x = torch.randn(V, generator=g) * 4
    x[torch.randint(0, V, (V // 8,), generator=g)] = 0.0
    x[torch.randint(0, V, (V // 8,), generator=g)] = -0.0
    x[torch.randint(0, V, (V // 8,), generator=g)] = -INF
    return x


@pytest.mark.parametrize("theta", [1.0, 0.7, 1.3])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 5])
def test_restatement_is_the_installed_processors_chain_bit_for_bit_in_fp32(theta, n):
    V = 37
    g = torch.Generator().manual_seed(1000 * n + int(theta * 10))
    lengths = sorted({0, 1, 2, 40, 300} | {max(n - 2, 0), max(n - 1, 0), n, n + 1})
    checked = 0
    for L_ in lengths:
        for dup in (False, True):
            for Lp in sorted({0, L_ // 2, L_}):
                h = _history(g, V, L_, dup)
                prompt, gen = h[:Lp], h[Lp:]
                x = _logits(g, V)
                for m in sorted({0, len(gen), len(gen) + 1}):            # m = 0, count = m, count = m - 1
                    for eos in (-1, int(h[0]) if h else 3, 5):
                        want = _hf(x, prompt, gen, theta, n, m, eos)
                        got = R.process_row(x, h, len(gen), theta, n, m, eos)
                        assert got.dtype == torch.float32
                        assert torch.equal(_bits(got), _bits(want)), (L_, dup, Lp, m, eos)
                        checked += 1
    assert checked >= 100


def test_restatement_edge_cases_by_hand():
    x = torch.tensor([2.0, -2.0, 0.0, -0.0, -INF, 3.0, 1.0, 6.0])
    # distinct ids once, however often they occur; -0 keeps its sign; -inf stays
    got = R.process_row(x, [0, 0, 1, 1, 1, 3, 4, 2], 8, repetition_penalty=2.0)
    assert torch.equal(_bits(got), _bits(torch.tensor([1.0, -4.0, 0.0, -0.0, -INF, 3.0, 1.0, 6.0])))
    got = R.process_row(x, [0, 1], 2, repetition_penalty=0.5)          # theta < 1 rewards
    assert got.tolist()[:2] == [4.0, -1.0]
    # n = 2, history 5 6 5 7 5: the suffix (5) was followed by 6 and by 7
    got = R.process_row(x, [5, 6, 5, 7, 5], 5, no_repeat_ngram_size=2)
    assert got[6] == -INF and got[7] == -INF and torch.equal(got[:6], x[:6])
    # L = n - 1 and L = n - 2: nothing to ban; L = n: one window, which needs its own first n - 1 ids to be the suffix
    assert torch.equal(R.process_row(x, [5, 6], 2, no_repeat_ngram_size=3), x)
    assert torch.equal(R.process_row(x, [5], 1, no_repeat_ngram_size=3), x)
    assert torch.equal(R.process_row(x, [5, 6, 7], 3, no_repeat_ngram_size=3), x)
    assert R.process_row(x, [5, 5, 5], 3, no_repeat_ngram_size=3)[5] == -INF
    # n = 1 bans every id of the history; an empty history bans nothing
    got = R.process_row(x, [0, 7, 7], 3, no_repeat_ngram_size=1)
    assert got[0] == -INF and got[7] == -INF and torch.equal(got[1:7], x[1:7])
    assert torch.equal(R.process_row(x, [], 0, 1.3, 1, 0, 2), x)
    # min_new_tokens counts generated tokens only; eos = -1 switches it off
    assert R.process_row(x, [1, 2, 3], 1, min_new_tokens=2, eos=5)[5] == -INF
    assert torch.equal(R.process_row(x, [1, 2, 3], 2, min_new_tokens=2, eos=5), x)
    assert torch.equal(R.process_row(x, [1, 2, 3], 0, min_new_tokens=2, eos=-1), x)
    # the order: the penalty sees the raw logit, the ban and eos overwrite it
    got = R.process_row(x, [7, 7], 2, 2.0, 1, 5, 0)
    assert got[7] == -INF and got[0] == -INF
    assert R.has_repeated_ngram([1, 2, 3, 1, 2], 2) and not R.has_repeated_ngram([1, 2, 3, 1, 2], 3)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_restatement_rounds_once_from_fp32_for_16_bit_logits(dtype):
    g = torch.Generator().manual_seed(7)
    x = (torch.randn(64, generator=g) * 4).to(dtype)
    h = list(range(0, 64, 2))
    got = R.process_row(x, h, len(h), repetition_penalty=1.3)
    assert got.dtype == dtype
    x64 = x.double()
    exact = torch.where(x64 < 0, x64 * float(torch.tensor(1.3, dtype=torch.float32)),
                        x64 / float(torch.tensor(1.3, dtype=torch.float32)))
    # the product / quotient of two fp32 numbers in double, rounded to fp32, IS the correctly rounded fp32 result (53 >=
    # 2 * 24 + 2 bits); then the one rounding to the 16-bit type
    want = exact.float().to(dtype)
    assert torch.equal(_bits(got[h]), _bits(want[h]))
    assert torch.equal(_bits(got[1::2]), _bits(x[1::2]))


# ---------------------------------------------------------------------------------------------------- the ABI --
def test_header_declares_the_entry_point_with_the_prototypes_arity_and_states_the_rule():
    src = open(HEADER).read()
    m = re.search(r"^int mk_logits_process\((.*?)\);", src, flags=re.M | re.S)
    assert m, "mk_logits_process is not declared in include/macaw_hip.h"
    assert len(m.group(1).split(",")) == len(L.SIGNATURES["mk_logits_process"]) == 19
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == 11 == L.ABI_VERSION
    for phrase in ("h_b = prompt_b ++ generated_b", "x = x < 0 ? x * theta : x / theta", "the division correctly rounded",
                   "Each distinct id is penalised once", "h[i .. i + n - 1) == h[L - n + 1 .. L)", "n = 1 bans every id",
                   "while n < m (generated tokens only), logit[eos] = -inf", "nothing is launched",
                   "V <= 2^18 = 262144"):
        assert phrase in src, phrase
    assert "logits_process.hip" in __import__("macaw_llm_amd.build", fromlist=["SOURCES"]).SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "logits_process.hip")).read()
    assert "asm" not in kernel                                          # plain loads and stores only


def test_the_library_exports_it_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    fn = lib.mk_logits_process
    sig = L.SIGNATURES["mk_logits_process"]
    assert fn(*[None if t is L._vp else t(0) for t in sig]) == -1      # null pointers: a code, nothing launched
    fake = 4096                                                         # never dereferenced: every call below is refused

    def call(logits=fake, ld=64, V=64, B=1, prompt=None, p_ld=0, P=0, p_len=None, out=fake, out_ld=8, n_max=8, n_dev=None,
             n_add=0, theta=1.3, n=2, m=0, eos=2, dtype=L.MK_F32):
        return fn(logits, ld, V, B, prompt, p_ld, P, p_len, out, out_ld, n_max, n_dev, n_add, theta, n, m, eos, dtype, None)

    for bad in (dict(logits=None), dict(out=None), dict(prompt=fake, P=4, p_ld=4), dict(theta=0.0), dict(theta=-1.0),
                dict(theta=float("nan")), dict(theta=float("inf")), dict(n=-1), dict(m=-1), dict(V=0), dict(B=0),
                dict(ld=63), dict(n_max=-1), dict(out_ld=7), dict(prompt=fake, p_len=fake, P=4, p_ld=3)):
        assert call(**bad) == -1, bad
    assert call(V=(1 << 18) + 1, ld=(1 << 18) + 1) == -2               # the bitmap's LDS budget
    assert call(dtype=L.MK_FP8) == -2
    # everything off: success without a launch (the pointers are not device memory)
    assert call(theta=1.0, n=0, m=0) == 0 and call(theta=1.0, n=0, m=5, eos=-1) == 0
    assert "mk_logits_process" in inspect.getsource(ops.logits_process)


# ------------------------------------------------------------------------------ public arguments and refusals --
def test_generate_and_set_logits_processors_carry_the_new_arguments():
    want = dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for k, v in want.items():
        assert p[k].default == v and type(p[k].default) is type(v), k
    p = inspect.signature(Mo.MM_LLMs.set_logits_processors).parameters
    assert {k: p[k].default for k in p} == want
    assert Mo.PROCESSORS[0] == want
    try:
        Mo.MM_LLMs.set_logits_processors(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8)
        assert Mo.PROCESSORS[0] == dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8)
        with pytest.raises(ValueError, match="repetition_penalty"):
            Mo.MM_LLMs.set_logits_processors(repetition_penalty=0.0)
        assert Mo.PROCESSORS[0]["no_repeat_ngram_size"] == 3            # a refused call changes nothing
    finally:
        Mo.MM_LLMs.set_logits_processors()
    assert Mo.PROCESSORS[0] == want
    fwd = inspect.getsource(Mo.MM_LLMs.forward)
    assert "**PROCESSORS[0]" in fwd and "**SAMPLING[0]" in fwd and "**BEAM_SEARCH[0]" in fwd


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4), **kw)


def test_every_refusal_names_its_argument_and_the_defaults_raise_nothing():
    for bad in (0.0, -1.0, float("nan"), float("inf"), "1.2", None, True):
        with pytest.raises(ValueError, match="repetition_penalty"):
            _generate(repetition_penalty=bad)
        with pytest.raises(ValueError, match="repetition_penalty"):
            Mo.MM_LLMs.set_logits_processors(repetition_penalty=bad)
    for name in ("no_repeat_ngram_size", "min_new_tokens"):
        for bad in (-1, 2.0, 1.5, "3", None, True):
            with pytest.raises(ValueError, match=name):
                _generate(**{name: bad})
            with pytest.raises(ValueError, match=name):
                Mo.MM_LLMs.set_logits_processors(**{name: bad})
    assert Mo.PROCESSORS[0] == dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)
    for on in (dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(min_new_tokens=4)):
        with pytest.raises(ValueError, match=f"{next(iter(on))}.*not built"):
            _generate(num_beams=2, **on)
        with pytest.raises(_PastTheChecks):                             # one beam: accepted
            _generate(num_beams=1, **on)
    with pytest.raises(_PastTheChecks):
        _generate(num_beams=1)
    with pytest.raises(_PastTheChecks):                                 # beams with the defaults: untouched
        _generate(num_beams=4)
    assert Mo._processors_check("generate", 1.0, 0, 0) is None and Mo._processors_check("generate", 1, 0, 0) is None
    assert Mo._processors_check("generate", 1.2, 3, 8) == (1.2, 3, 8)
    # the refusal lives in generate, not in beam_check, whose signature other tests pin
    from macaw_llm_amd import beam
    assert "repetition_penalty" not in inspect.getsource(beam)


def test_the_processors_sit_in_front_of_every_selection(monkeypatch):
    for loop in ("graph", "cached", "nocache"):
        for sampled in (False, True):
            _processors_in_front(monkeypatch, loop, sampled)


def _processors_in_front(monkeypatch, loop, sampled):
    """read off generate()'s own launch log (tests/test_generate_trace_cpu.py): on the graph loop, the cached eager loop
    and the use_cache=False loop every selection -- decode_emit / decode_emit_sample, argmax_rows / sample_rows -- has
    ops.logits_process directly in front of it, on the same logits; the graph loop hands it the emit's output matrix
    and the device's column counter, the eager loops the ids they have selected so far and the count from the host"""
    import test_generate_trace_cpu as T
    more = {"graph": {}, "cached": dict(decode_graph=False), "nocache": dict(use_cache=False)}[loop]
    with monkeypatch.context() as mp:
        got = T.run_trace_case(dict(N=12, finish=None, kw={**T.PROC, **(T.SAMPLE if sampled else {}), **more}), mp)
    log = [e for e in got["log"] if not isinstance(e, str)]
    want = {("graph", False): "decode_emit", ("graph", True): "decode_emit_sample"}.get((loop, sampled),
                                                                                          "sample_rows" if sampled else "argmax_rows")
    picks = [i for i, e in enumerate(log) if e[0] in ("decode_emit", "decode_emit_sample", "argmax_rows", "sample_rows")]
    assert {log[i][0] for i in picks} == {want} and len(picks) == (3 if loop == "graph" else 12)   # (eager, eager, captured)
    ids = got["returns"][0][2]
    for t, i in enumerate(picks):
        name, logits, _, out, n_dev, n_add = log[i - 1][:6]
        assert name == "logits_process" and logits == log[i][1]
        if loop == "graph":
            assert n_add == 0 and n_dev.endswith(f"={[t]}".replace(" ", "")) and out == log[i][7]      # column t of the emit's matrix
        else:
            assert (n_dev, n_add) == (None, t)
            have = [row[:t] + [0] * (12 - t) for row in ids]            # the ids selected so far, pad behind them
            assert out.endswith("=" + str(have).replace(" ", ""))
