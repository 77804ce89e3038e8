"""CPU: prompt-lookup speculative decoding -- the rule of include/macaw_hip.h as restated in tests/spec_ref.py on
hand-written cases, the draft against transformers' own PromptLookupCandidateGenerator, the verify step and the whole
loop (simulate), the ABI of the three new entry points, the public arguments and every refusal, the launch sequence of a
verify step of the layer (the fake-ops technique of tests/test_decode_trace_cpu.py) and the decode loop on recorders."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import spec_ref as R
from test_beam_cpu import BeamTrace, _FakeCapture, _FakeGraph
from test_decode_trace_cpu import _t

from macaw_llm_amd import engine as eng
from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
I32, F32 = torch.int32, torch.float32


# --------------------------------------------------------------------------------------------- 1. the draft --
def test_lookup_hand_written_cases():
    # the largest n wins: the 2-gram (1, 2) occurs at 0 (-> 3), the 1-gram (2) also at 5 (-> 9) -- n = 2 decides
    assert R.lookup([1, 2, 3, 4, 7, 2, 9, 1, 2], 3, 2) == [3, 4, 7]
    assert R.lookup([1, 2, 3, 4, 7, 2, 9, 1, 2], 3, 1) == [3, 4, 7]          # n = 1: the earliest 2 is at 1
    assert R.lookup([5, 2, 8, 1, 2, 3, 9, 2], 2, 1) == [8, 1]                # the earliest match wins, not the latest
    assert R.lookup([1, 2, 8, 8, 1, 2, 9, 9, 1, 2], 2, 2) == [8, 8]
    # the trailing window itself is never a match: (3, 4) occurs only at the end; n = 1 finds nothing either
    assert R.lookup([1, 2, 3, 4], 4, 2) == []
    assert R.lookup([4, 4], 3, 2) == [4]                                     # n = 1: window 0 matches, continuation cut at L
    # the continuation is cut at L
    assert R.lookup([1, 2, 3, 1, 2], 8, 2) == [3, 1, 2]
    assert R.lookup([7, 1, 7], 15, 5) == [1, 7]
    # no 2-gram match: falls to n = 1
    assert R.lookup([1, 2, 3, 9, 2], 2, 2) == [3, 9]
    # an eos at draft position 0: no draft, and no retry at the smaller n (n = 1 alone proposes [5, 6, 1])
    assert R.lookup([2, 5, 6, 1, 2, 0, 3, 1, 2], 3, 2, eos=0) == []
    assert R.lookup([2, 5, 6, 1, 2, 0, 3, 1, 2], 3, 1, eos=0) == [5, 6, 1]
    assert R.lookup([1, 2, 3, 0, 4, 1, 2], 4, 2, eos=0) == [3]               # cut BEFORE the first eos
    assert R.lookup([1, 2, 3, 0, 4, 1, 2], 4, 2, eos=-1) == [3, 0, 4, 1]     # eos = -1 never matches
    # L < 2
    assert R.lookup([], 4, 2) == [] and R.lookup([3], 4, 2) == []
    # ids outside the vocabulary never match and are never proposed
    assert R.lookup([50, 1, 7, 50, 1], 3, 2, V=40) == [7]                    # n = 2 holds 50: skipped; n = 1 -> [7], cut at 50
    assert R.lookup([50, 7, 8, 50], 3, 1, V=40) == []                        # the tail itself is outside
    assert R.lookup([-1, 7, -1, 3, 4, 3], 3, 2, V=40) == [4, 3]
    assert R.lookup([3, -1, 9, 3], 3, 1, V=40) == []                         # first proposed id outside: nothing, no retry


def test_lookup_is_transformers_prompt_lookup_candidate_generator():
    try:
        from transformers.generation.candidate_generator import PromptLookupCandidateGenerator
    except ImportError:
        pytest.skip("this transformers does not export PromptLookupCandidateGenerator")
    g = np.random.default_rng(0)
    hits = 0
    for case in range(400):
        Ln, G, n = int(g.integers(1, 14)), int(g.integers(1, 8)), int(g.integers(1, 5))
        h = g.integers(0, 5, size=Ln).tolist()
        eos = int(g.integers(0, 5)) if case % 3 else None
        gen = PromptLookupCandidateGenerator(eos_token_id=None if eos is None else torch.tensor([eos]), num_output_tokens=G,
                                             max_matching_ngram_size=n, max_length=10 ** 6)
        cand, _ = gen.get_candidates(torch.tensor([h]))
        want = cand[0, Ln:].tolist()
        got = R.lookup(h, G, n, -1 if eos is None else eos)
        assert got == want, (h, G, n, eos, got, want)
        hits += bool(got)
    assert hits > 150                                                        # matches are frequent over five ids


# ------------------------------------------------------------------------------------ 2. verify and the loop --
def _books(G, max_new, tok, n_draft, n_out=0, pos=10, out=None, pad=0):
    bk = R.Books(G, max_new, pad, pos)
    bk.tok, bk.n_draft, bk.n_out = list(tok), n_draft, n_out
    if out:
        bk.out[:len(out)] = out
    return bk


def test_verify_hand_written_cases():
    # partial accept: draft (5, 6, 7), the model says 5, 6, 9, ... -> emits 5, 6, 9
    bk = _books(3, 20, [4, 5, 6, 7], 3, n_out=2, out=[1, 4])
    assert R.verify(bk, [5, 6, 9, 1]) == 3
    assert (bk.out[:5], bk.n_out, bk.pos, bk.steps, bk.done, bk.tok[0]) == ([1, 4, 5, 6, 9], 5, 13, 1, False, 9)
    # full accept plus the bonus token
    bk = _books(3, 20, [4, 5, 6, 7], 3)
    assert R.verify(bk, [5, 6, 7, 8]) == 4 and bk.out[:4] == [5, 6, 7, 8] and bk.tok[0] == 8 and bk.pos == 14
    # nothing accepted: one token, as plain greedy; columns behind n_draft are not compared
    bk = _books(3, 20, [4, 5, 0, 0], 1)
    assert R.verify(bk, [9, 0, 0, 0]) == 1 and bk.out[:1] == [9]
    bk = _books(3, 20, [4, 5, 0, 0], 1)
    assert R.verify(bk, [5, 0, 0, 3]) == 2 and bk.out[:2] == [5, 0]          # the pad column equals a_1 = 0: not a draft
    # an eos inside an accepted run: cut after it, inclusive
    bk = _books(3, 20, [4, 5, 2, 7], 3)
    assert R.verify(bk, [5, 2, 7, 8], eos=2) == 2
    assert (bk.out[:3], bk.n_out, bk.done, bk.tok[0], bk.pos) == ([5, 2, 0], 2, True, 2, 12)
    # the max_new_tokens cut
    bk = _books(3, 6, [4, 5, 6, 7], 3, n_out=4, out=[1, 1, 1, 4])
    assert R.verify(bk, [5, 6, 7, 8]) == 2 and bk.out == [1, 1, 1, 4, 5, 6] and bk.done and bk.tok[0] == 6
    # a finished sample changes nothing
    before = bk.fields()
    assert R.verify(bk, [5, 6, 7, 8]) == 0 and bk.fields() == before
    R.draft_into(bk, [1, 4, 5], 2)
    assert bk.n_draft == 0 and bk.tok[1:] == [0, 0, 0]
    # token 0: one row, the draft is not read
    bk = _books(3, 20, [0, 9, 9, 9], 3, pos=6)
    assert R.verify(bk, [9]) == 1 and (bk.out[0], bk.pos, bk.steps) == (9, 7, 1)


def test_simulate_hand_written_cases():
    # cold: nothing repeats, one token per step
    assert R.simulate([], [1, 2, 3, 4, 5], 4, 2, -1, 5) == ([1] * 5, 5)
    # the history holds the answer: token 0, then 1 + 4 per step while the draft is right
    hist = [10, 11] + list(range(20, 32)) + [10, 11]
    counts, steps = R.simulate(hist, list(range(20, 32)), 4, 2, -1, 12)
    assert counts == [1, 5, 5, 1] and steps == 4
    # partial accept: the model leaves the history's continuation after two tokens
    counts, steps = R.simulate([1, 2, 3, 4, 5, 6, 1], [2, 3, 9, 8, 7], 4, 1, -1, 5)
    assert counts == [1, 2, 1, 1] and steps == 4
    # an eos inside an accepted run ends the sample there
    counts, steps = R.simulate(hist, list(range(20, 25)), 4, 2, 24, 12)
    assert counts == [1, 4] and steps == 2
    # the max_new_tokens cut: the second step could emit 5 and is cut to 3
    counts, steps = R.simulate(hist, list(range(20, 24)), 4, 2, -1, 4)
    assert counts == [1, 3] and steps == 2
    # a loop that repeats its own output accepts from the generated tokens alone
    counts, steps = R.simulate([], [1, 2, 1, 2, 1, 2, 1, 2], 2, 2, -1, 8)
    assert counts == [1, 1, 1, 3, 2] and steps == 5


# ------------------------------------------------------------------------------------------------ 3. the ABI --
NEW = {"mk_spec_lookup": 18, "mk_spec_verify_emit": 18, "mk_decode_step_attn_multi": 21}


def test_header_declares_the_three_entry_points_states_the_rule_and_keeps_abi_11():
    src = open(HEADER).read()
    for name, arity in NEW.items():
        m = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/macaw_hip.h"
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == arity, name
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == 11 == L.ABI_VERSION
    for phrase in ("take the SMALLEST i with i + n < L", "cut the draft BEFORE its first eos", "no smaller n is tried",
                   "Ids outside [0, V) never match", "A = the number of leading draft tokens", "A finished sample changes nothing",
                   "BIT FOR BIT", "no batch-wide counter"):
        assert phrase in src, phrase
    from macaw_llm_amd import build
    assert "spec.hip" in build.SOURCES
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "spec.hip")).read()
    assert "asm" not in kernel                                           # plain loads and stores only


def test_the_library_exports_them_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    assert lib.mk_abi_version() == 11
    for name in NEW:                                                     # null pointers: a code, nothing launched
        assert getattr(lib, name)(*[None if t is L._vp else t(0) for t in L.SIGNATURES[name]]) == -1, name
    fake = 4096                                                          # never dereferenced: every call below is refused

    def look(prompt=None, p_ld=0, P=0, p_len=None, out=fake, out_ld=8, n_max=8, n_out=fake, done=fake, tok=fake,
             n_draft=fake, B=2, G=4, n=2, V=40, pad=0, eos=2):
        return lib.mk_spec_lookup(prompt, p_ld, P, p_len, out, out_ld, n_max, n_out, done, tok, n_draft, B, G, n, V, pad,
                                  eos, None)

    for bad in (dict(out=None), dict(n_out=None), dict(done=None), dict(tok=None), dict(n_draft=None), dict(B=0), dict(G=0),
                dict(G=16), dict(n=0), dict(V=0), dict(n_max=-1), dict(out_ld=7), dict(prompt=fake, P=4, p_ld=4),
                dict(prompt=fake, p_len=fake, P=4, p_ld=3), dict(prompt=fake, p_len=fake, P=-1)):
        assert look(**bad) == -1, bad

    def ver(logits=fake, ld=40, V=40, B=2, R=5, Q=5, eos=2, tok=fake, n_draft=fake, pos=fake, n_out=fake, done=fake,
            out=fake, out_ld=8, n_max=8, steps=fake, dtype=L.MK_BF16):
        return lib.mk_spec_verify_emit(logits, ld, V, B, R, Q, eos, tok, n_draft, pos, n_out, done, out, out_ld, n_max,
                                       steps, dtype, None)

    for bad in (dict(logits=None), dict(tok=None), dict(n_draft=None), dict(pos=None), dict(n_out=None), dict(done=None),
                dict(out=None), dict(steps=None), dict(V=0), dict(B=0), dict(ld=39), dict(Q=0), dict(Q=17, R=17), dict(R=2),
                dict(n_max=-1), dict(out_ld=7)):
        assert ver(**bad) == -1, bad
    assert ver(dtype=L.MK_FP8) == -2

    def att(q=fake, k=fake, v=fake, in_bs=384, cos=fake, sin=fake, kc=fake, vc=fake, kv_ld=256, kv_bs=256 * 12, o=fake,
            o_bs=128, pos=fake, t_max=12, B=2, Q=5, H=2, hd=64, dtype=L.MK_BF16):
        return lib.mk_decode_step_attn_multi(q, k, v, in_bs, cos, sin, kc, vc, kv_ld, kv_bs, o, o_bs, pos, t_max, B, Q, H,
                                             hd, 0.125, dtype, None)

    for bad in (dict(q=None), dict(k=None), dict(v=None), dict(cos=None), dict(sin=None), dict(kc=None), dict(vc=None),
                dict(o=None), dict(pos=None), dict(B=0), dict(H=0), dict(t_max=0), dict(Q=0)):
        assert att(**bad) == -1, bad
    for bad in (dict(Q=17), dict(hd=48), dict(dtype=L.MK_F32), dict(q=fake + 8), dict(pos=fake + 2), dict(in_bs=385),
                dict(kv_ld=257)):
        assert att(**bad) == -2, bad
    for name, op in (("mk_spec_lookup", ops.spec_lookup), ("mk_spec_verify_emit", ops.spec_verify_emit),
                     ("mk_decode_step_attn_multi", ops.decode_step_attn_multi)):
        assert name in inspect.getsource(op)


def test_spec_attn_ok_is_the_entry_points_domain():
    ok = ops.spec_attn_ok
    for hd in (16, 32, 64, 128):
        assert ok(torch.bfloat16, hd, 4096, 16) and ok(torch.float16, hd, 1, 1)
    assert not ok(torch.float32, 64, 64, 4) and not ok(torch.bfloat16, 48, 64, 4)
    assert not ok(torch.bfloat16, 64, 64, 17) and not ok(torch.bfloat16, 64, 64, 0) and not ok(torch.bfloat16, 64, 0, 4)
    s = ops.SpecState(3, 4, 12, 9, "cpu")
    assert (s.B, s.G, s.Q, s.n_max, s.pad) == (3, 4, 5, 12, 9)
    assert tuple(s.out.shape) == (3, 12) and tuple(s.tok.shape) == (3, 5) and bool((s.out == 9).all()) and bool((s.tok == 9).all())
    for t in (s.pos, s.n_out, s.n_draft, s.steps):
        assert t.dtype == I32 and tuple(t.shape) == (3,) and not bool(t.any())
    assert s.done.dtype == torch.bool and s.out.dtype == s.tok.dtype == torch.long


# ------------------------------------------------------------------------------ 4. public arguments, refusals --
def test_generate_and_set_prompt_lookup_carry_the_new_arguments():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    want = dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=2, return_lookup_stats=False)
    for k, v in want.items():
        assert p[k].default == v and type(p[k].default) is type(v), k
    p = inspect.signature(Mo.MM_LLMs.set_prompt_lookup).parameters
    assert {k: p[k].default for k in p} == dict(num_tokens=None, max_matching_ngram_size=2)
    off = dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=2)
    assert Mo.PROMPT_LOOKUP[0] == off
    try:
        Mo.MM_LLMs.set_prompt_lookup(7, max_matching_ngram_size=3)
        assert Mo.PROMPT_LOOKUP[0] == dict(prompt_lookup_num_tokens=7, max_matching_ngram_size=3)
        for bad in (16, -1, 2.0, "4", True):
            with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
                Mo.MM_LLMs.set_prompt_lookup(bad)
        for bad in (0, -1, 1.5, None, True):
            with pytest.raises(ValueError, match="max_matching_ngram_size"):
                Mo.MM_LLMs.set_prompt_lookup(4, bad)
        assert Mo.PROMPT_LOOKUP[0]["prompt_lookup_num_tokens"] == 7          # a refused call changes nothing
        Mo.MM_LLMs.set_prompt_lookup(0)
        assert Mo.PROMPT_LOOKUP[0] == off                                    # 0 is off
    finally:
        Mo.MM_LLMs.set_prompt_lookup()
    assert Mo.PROMPT_LOOKUP[0] == off
    fwd = inspect.getsource(Mo.MM_LLMs.forward)
    assert 'input_ids=inputs["input_ids"], **PROMPT_LOOKUP[0]' in fwd and "**PROCESSORS[0], **look)" in fwd


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates what it can before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(B=1, dtype=torch.bfloat16, **kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(B, 2, 4, dtype=dtype), **kw)


def test_every_refusal_raises_through_generate_and_names_its_condition():
    for bad in (16, -1, 2.0, "4", True):
        with pytest.raises(ValueError, match="prompt_lookup_num_tokens"):
            _generate(prompt_lookup_num_tokens=bad)
    for bad in (0, -1, 1.5, None, True):
        with pytest.raises(ValueError, match="max_matching_ngram_size"):
            _generate(prompt_lookup_num_tokens=4, max_matching_ngram_size=bad)
    cases = [(dict(num_beams=2), "num_beams=2"), (dict(do_sample=True), "do_sample=True"),
             (dict(repetition_penalty=1.2), "logits processor"), (dict(no_repeat_ngram_size=2), "logits processor"),
             (dict(min_new_tokens=3), "logits processor"), (dict(kv_cache="fp8"), "kv_cache='fp8'"),
             (dict(use_cache=False), "use_cache=False"),
             (dict(attention_mask=torch.tensor([[0, 1]])), "padded attention_mask"),
             (dict(B=7), r"B x \(G \+ 1\) = 7 x 5 = 35"), (dict(dtype=torch.float32), "fp32 parameters")]
    for kw, what in cases:
        with pytest.raises(ValueError, match=rf"prompt_lookup_num_tokens=4.*{what}.*not built"):
            _generate(prompt_lookup_num_tokens=4, **kw)
        kw = {k: v for k, v in kw.items()}
        for off in (None, 0):                                            # off: none of them is refused here
            with pytest.raises(_PastTheChecks):
                _generate(prompt_lookup_num_tokens=off, **{k: v for k, v in kw.items() if k != "kv_cache"})
    with pytest.raises(_PastTheChecks):                                  # on, inside every limit: accepted
        _generate(prompt_lookup_num_tokens=15, B=2, attention_mask=torch.ones(2, 2, dtype=torch.long))
    with pytest.raises(_PastTheChecks):
        _generate(prompt_lookup_num_tokens=4, B=6, dtype=torch.float16, max_matching_ngram_size=9)


def test_the_shape_check_behind_the_model_asks_spec_attn_ok_about_the_cache_rows_and_the_step_rows(monkeypatch):
    """ops.spec_attn_ok(dtype, head size, Tmax = S0 + max_new_tokens + G, G + 1): a head size outside it is refused with
    exactly those numbers, before anything is launched"""
    from transformers import LlamaConfig
    lm = Mo.LlamaForCausalLM(LlamaConfig(hidden_size=96, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2,
                                         num_key_value_heads=2, vocab_size=40, max_position_embeddings=64)).to(torch.bfloat16)
    monkeypatch.setattr(Mo, "_dev_check", lambda t: None)
    asked = []
    real = ops.spec_attn_ok
    monkeypatch.setattr(ops, "spec_attn_ok", lambda *a: asked.append(a) or real(*a))
    with pytest.raises(ValueError, match=r"prompt_lookup_num_tokens=4.*spec_attn_ok is false for head size 48, 21 positions "
                                         r"and 5 rows.*not built"):
        lm.generate(inputs_embeds=torch.zeros(2, 5, 96, dtype=torch.bfloat16), max_new_tokens=12, prompt_lookup_num_tokens=4)
    assert asked == [(torch.bfloat16, 48, 5 + 12 + 4, 4 + 1)]


# ------------------------------------------------------------------- 5. the launch sequence of a verify step --
def _layer_case(monkeypatch, weights, B=2, Q=5, D=128, FF=256, hd=64, TMAX=24, fused=True, **kw):
    H, M = D // hd, B * Q
    tr = BeamTrace(monkeypatch)
    seen = []
    monkeypatch.setattr(ops, "decode_step_attn_multi",
                        lambda *a, **k: seen.append((a, k)) or tr.calls.append(("decode_step_attn_multi", {})) or a[13])
    x2 = _t(M, D)
    wqkv, wgu = _t(3 * D, D), _t(2 * FF, D)
    wq, wk, wv, wg, wu = wqkv[:D], wqkv[D:2 * D], wqkv[2 * D:], wgu[:FF], wgu[FF:]
    wo, wd, ln1, ln2 = _t(D, D), _t(D, FF), _t(D), _t(D)
    q8 = lambda N, Kd: (_t(N, Kd, dtype=torch.uint8), _t(N, dtype=F32))  # noqa: E731
    w8 = None if weights == "w16" else (q8(3 * D, D), q8(D, D), q8(2 * FF, D), q8(D, FF))
    kvc, pos = _t(B, TMAX, 2 * D), _t(B, dtype=I32)
    args = dict(t_dev=pos, w8=w8, spec=eng.Spec(pos, Q))
    args.update(kw)
    out = eng.llama_layer_cached(x2, B, Q, 0, kvc, TMAX, pos, _t(TMAX, hd), _t(TMAX, hd), H, 1e-6, wq, wk, wv, wo, wg, wu,
                                 wd, ln1, ln2, wqkv if fused else None, wgu if fused else None, **args)
    assert tuple(out.shape) == (M, D)
    return tr.calls, seen, dict(kvc=kvc, pos=pos, B=B, Q=Q, H=H, hd=hd, TMAX=TMAX, D=D)


@pytest.mark.parametrize("weights,lin", [("w16", "decode_linear"), ("fp8", "decode_linear_fp8")])
def test_verify_step_of_the_layer_is_the_five_launches_with_the_multi_query_attention(monkeypatch, weights, lin):
    calls, seen, c = _layer_case(monkeypatch, weights)
    assert [n for n, _ in calls] == [lin, "decode_step_attn_multi", lin, lin, lin]
    assert [a["prologue"] for n, a in calls if n == lin] == [1, 0, 1, 2]
    for n, a in calls:                                                   # every weight stream sees the B * Q token rows
        if n == lin:
            assert a["x"].shape[0] == c["B"] * c["Q"]
    (a, k), = seen
    q, kn, vn, in_bs, cos, sin, cache, pos, t_max, B, Q, H, hd, out, scale = a
    assert q is kn is vn and tuple(q.shape) == (c["B"] * c["Q"], 3 * c["D"]) and in_bs == 3 * c["D"]
    assert cache is c["kvc"] and pos is c["pos"] and (t_max, B, Q, H, hd) == (c["TMAX"], c["B"], c["Q"], c["H"], c["hd"])
    assert k == dict(k_off=c["D"], v_off=2 * c["D"]) and tuple(out.shape) == (c["B"] * c["Q"], c["D"])


def test_verify_step_on_unfused_storage_takes_the_general_path_with_the_multi_query_attention(monkeypatch):
    calls, seen, c = _layer_case(monkeypatch, "w16", fused=False)
    names = [n for n, _ in calls]
    assert names.count("decode_step_attn_multi") == 1 and "decode_step_attn" not in names
    assert "rope_" not in names and "copy2d" not in names


def test_spec_refuses_what_it_does_not_compose_with(monkeypatch):
    pos = _t(2, dtype=I32)
    for kw in (dict(ragged=eng.Ragged(_t(2, 5, dtype=I32), _t(2, 5, dtype=I32), _t(2, dtype=I32))),
               dict(kv8=_t(2, 24, 4, dtype=F32)), dict(beam=eng.Beam(_t(10, 7, dtype=I32), 5, 5)),
               dict(t_dev=None),                                         # a host position
               dict(spec=eng.Spec(pos, 4))):                             # rows != B * Q
        with pytest.raises(ValueError, match="spec takes"):
            _layer_case(monkeypatch, "w16", **kw)
    assert inspect.signature(eng.llama_layer_cached).parameters["spec"].default is None


# --------------------------------------------------------------------------------- 6. the decode loop on recorders --
@pytest.mark.parametrize("graph", [True, False], ids=["graph", "loop"])
@pytest.mark.parametrize("N", [1, 2, 12])
def test_lookup_loop_verifies_once_from_the_prefill_then_runs_one_fixed_step(monkeypatch, graph, N):
    """token 0 from the prefill's B rows, then per step lookup -> embedding of the [B, Q] ids -> layers (engine.Spec on
    the state's own positions) -> logits -> verify; on the graph path one eager step, one captured step, then replays
    only.  The fake verify emits one token per step, so the loop runs its longest: N - 1 steps."""
    B, G, S0, V, D = 2, 4, 5, 40, 16
    Q = G + 1
    log = _FakeGraph.log = []
    monkeypatch.setattr(torch.cuda, "CUDAGraph", _FakeGraph)
    monkeypatch.setattr(torch.cuda, "graph", _FakeCapture)
    seen = {}

    def emb(table, ids):
        log.append(("embedding_fwd", tuple(ids.shape)))
        assert ids.data_ptr() == seen["ss"].tok.data_ptr()
        return torch.zeros(ids.numel(), D)

    def lookup(ss, V_, n, eos, prompt=None, prompt_len=None):
        log.append(("spec_lookup", n, eos, prompt, prompt_len))
        assert ss is seen["ss"]

    def verify(logits, V_, eos, ss):
        log.append(("spec_verify_emit", tuple(logits.shape), eos))
        if "ss" not in seen:
            assert ss.pos.tolist() == [S0 - 1] * B                       # token 0 advances it to S0
        seen["ss"] = ss
        ss.n_out += 1
        ss.pos += 1
        ss.done |= ss.n_out >= ss.n_max

    def run(x, Sn, t0, pos=None, t_dev=None, beam=None, spec=None):
        log.append(("run", tuple(x.shape), Sn, spec.Q))
        assert spec.pos is seen["ss"].pos and t_dev is spec.pos and beam is None
        return x

    monkeypatch.setattr(ops, "embedding_fwd", emb)
    monkeypatch.setattr(ops, "spec_lookup", lookup)
    monkeypatch.setattr(ops, "spec_verify_emit", verify)

    class Head:
        weight = torch.zeros(V, D)

    class Fake:
        lm_head = Head()
    ids, steps = Mo.LlamaForCausalLM._generate_lookup.__wrapped__(
        Fake(), run, lambda h: torch.zeros(h.shape[0], V), torch.zeros(B, D), None, B, G, S0, N, 7, 0, "cpu", 3, "H", "HL",
        graph)
    step = [("spec_lookup", 3, 7, "H", "HL"), ("embedding_fwd", (B * Q,)), ("run", (B * Q, D), Q, Q),
            ("spec_verify_emit", (B * Q, V), 7)]
    first = [("spec_verify_emit", (B, V), 7)]
    if not graph or N <= 2:
        assert log == first + step * (N - 1)
    else:
        assert log == first + step + ["capture{"] + step + ["}"] + ["replay"] * (N - 2)
    assert tuple(ids.shape) == (B, min(N, seen["ss"].n_out.max().item())) and tuple(steps.shape) == (B,) and steps.dtype == I32
    # (engine.Spec on the state's positions with Q = G + 1 rows: asserted in run() above; the look at the done flags
    # after every 8th replay: test_beam_cpu.py's test of modeling._decode_steps, the one driver under this loop)
