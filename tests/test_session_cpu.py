"""CPU: the surface of generate(session=, return_session=True) -- the header's rule, the ctypes prototype and the ABI
version of mk_flash_attn_varlen_fwd, the public arguments, MM_LLMs.set_session, the refusals that need no model (each
naming its condition), the engine's guard, and GenerateSession's bookkeeping on hand-made books: the final token by eos,
by stop sequence and by max_new_tokens, pads excluded."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

from macaw_llm_amd import engine as eng
from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")


# --------------------------------------------------------------------------------------- ABI and signatures --
def test_the_header_declares_the_entry_point_documents_the_rule_and_the_abi_stays_11():
    src = open(HEADER).read()
    m = re.search(r"\nint mk_flash_attn_varlen_fwd\(([^;]*)\);", src)
    assert m, "include/macaw_hip.h does not declare mk_flash_attn_varlen_fwd"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1)).replace("\n", " ").split(",")]
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["q", "k", "v", "o", "lse", "q_len", "k_len", "B", "H", "Lq", "Lk", "hd", "q_ld", "q_bs", "k_ld", "k_bs",
                     "v_ld", "v_bs", "o_ld", "o_bs", "scale", "dtype", "stream"]
    kinds = {"void*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "int64_t": C.c_int64, "int32_t": C.c_int32,
             "float": C.c_float}
    want = [kinds[re.sub(r"\bconst\b", "", " ".join(p.split()[:-1])).replace(" ", "")] for p in params]
    assert L.SIGNATURES["mk_flash_attn_varlen_fwd"] == want and len(want) == 23
    assert re.search(r"#define MK_ABI_VERSION 11\b", src) and L.ABI_VERSION == 11
    doc = " ".join(src[src.index("mk_flash_attn_fwd, always causal"):m.start()].replace(" * ", " ").split())
    for phrase in ("ql_b = clamp(q_len[b], 0, Lq)", "kl_b = clamp(k_len[b], 0, Lk)", "j < kl_b and j <= i + (kl_b - ql_b)",
                   "o = 0 and lse = -inf", "no byte of k or v at a row >= kl_b is read", "the host never synchronises",
                   "MK_ERR_UNSUPPORTED", "MK_ERR_BAD_ARG", "there is no backward",
                   "up to and including the sample's final token", "pads behind it never enter",
                   "what a fresh call would return for that sample alone", "emitted but never fed",
                   "pending token and becomes row 0", "no extra step is run for it"):
        assert phrase in doc, phrase
    if os.path.exists(L.LIB_PATH):
        assert L.load().mk_abi_version() == 11 and hasattr(L.load(), "mk_flash_attn_varlen_fwd")


def test_generate_takes_the_session_arguments_as_real_parameters_and_the_layer_signature_is_unchanged():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    for name, default in (("session", None), ("return_session", False), ("session_capacity", None)):
        assert name in p and p[name].default is default
        assert p[name].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD      # not swallowed by **_
    # the Chunk travels in place of a Ragged: every other caller binds to the signature it always had
    assert list(inspect.signature(eng.llama_layer_cached).parameters)[-6:] == ["t_dev", "w8", "kv8", "ragged", "beam", "spec"]
    assert eng.Chunk._fields == ("q_len", "k_len", "slot", "Lk", "q_host", "k_host")
    assert list(inspect.signature(ops.flash_attn_varlen_fwd).parameters) == [
        "q", "k", "v", "o", "q_len", "k_len", "B", "H", "Lq", "Lk", "hd", "q_ld", "q_bs", "k_ld", "k_bs", "v_ld", "v_bs", "o_ld",
        "o_bs", "scale", "lse", "q_off", "k_off", "v_off", "o_off"]
    for dt in (torch.bfloat16, torch.float16):
        assert ops.flash_varlen_ok(dt, 64) and ops.flash_varlen_ok(dt, 128)
        assert not ops.flash_varlen_ok(dt, 32) and not ops.flash_varlen_ok(dt, 48)
    assert not ops.flash_varlen_ok(torch.float32, 64)
    doc = " ".join(Mo.LlamaForCausalLM.generate.__doc__.split())
    for phrase in ("return_session=True and session=s", "up to and including the sample's final token",
                   "what a fresh call would return for that sample alone", "pending token and becomes row 0",
                   "ops.flash_attn_varlen_fwd", "engine.chunk_layout", "pass another seed per turn"):
        assert phrase in doc, phrase
    cls = " ".join(Mo.GenerateSession.__doc__.split())
    assert "pending token" in cls and "never fed" in cls


def test_set_session_reaches_generate_only_when_on_and_a_follow_up_turn_skips_the_towers():
    assert Mo.SESSION == [False]
    seen = []

    class LLM:
        _lora = None

        def generate(self, **kw):
            seen.append(kw)
            return "ids"

    class Fake:
        llm = LLM()

        def _param_dtype(self):
            return torch.bfloat16

        def prepare_inputs_for_generation(self, inputs):
            seen.append("prepare")
            return "emb", None, None
    try:
        assert Mo.MM_LLMs.forward(Fake(), {"inference": True}) == "ids"
        assert "return_session" not in seen[-1] and "session" not in seen[-1]
        Mo.MM_LLMs.set_session(True)
        assert Mo.SESSION == [True]
        del seen[:]
        Mo.MM_LLMs.forward(Fake(), {"inference": True})
        assert seen[0] == "prepare" and seen[-1]["return_session"] is True and "session" not in seen[-1]
        for k in ("images", "audios", "videos"):
            with pytest.raises(ValueError, match=f"{k} next to inputs\\['session'\\].*not built"):
                Mo.MM_LLMs.forward(Fake(), {"inference": True, "session": object(), k: torch.zeros(1)})
        Mo.MM_LLMs.set_session()
    finally:
        Mo.MM_LLMs.set_session()
    assert Mo.SESSION == [False]


# ------------------------------------------------------------------------------------------------ refusals --
class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(**kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(1, 2, 4, dtype=torch.bfloat16), **kw)


def _session():
    return Mo.GenerateSession([torch.zeros(1, 8, 8, dtype=torch.bfloat16)], [3], torch.tensor([5]), [[1, 2, 3, 5]], 4,
                              torch.device("cpu"))


def test_the_refusals_that_need_no_model_name_their_condition_and_the_default_raises_nothing():
    for how, kw in (("return_session=True", dict(return_session=True)), ("session=", dict(session=_session()))):
        where = re.escape(f"generate({how})")
        with pytest.raises(ValueError, match=where + " with use_cache=False"):
            _generate(use_cache=False, **kw)
        with pytest.raises(ValueError, match=where + " with num_beams=3.*not built"):
            _generate(num_beams=3, **kw)
        with pytest.raises(ValueError, match=where + " with num_samples=2.*not built"):
            _generate(num_samples=2, do_sample=True, **kw)
        with pytest.raises(ValueError, match=where + " with prompt_lookup_num_tokens=4.*not built"):
            _generate(prompt_lookup_num_tokens=4, **kw)
        with pytest.raises(ValueError, match=where + " with guidance_scale=1.5.*not built"):
            _generate(guidance_scale=1.5, negative_prompt_ids=torch.zeros(1, 2, dtype=torch.long), **kw)
        with pytest.raises(ValueError, match=where + " with kv_cache='fp8'.*no quantised attention over several new positions"):
            _generate(kv_cache="fp8", **kw)
        for bad in (0, -4, 2.5, "64", True):
            with pytest.raises(ValueError, match="session_capacity must be None or an integer >= 1"):
                _generate(session_capacity=bad, **kw)
        for ok in (dict(), dict(do_sample=True, seed=3), dict(decode_weights="fp8"), dict(repetition_penalty=1.3),
                   dict(stop_sequences=[[4, 5]]), dict(return_logprobs=True), dict(session_capacity=64),
                   dict(guidance_scale=1.0), dict(num_samples=1), dict(decode_graph=False)):
            with pytest.raises(_PastTheChecks):
                _generate(**ok, **kw)
    for other in ("a session", 7, {"cache": None}, [_session()]):
        with pytest.raises(ValueError, match=r"generate\(session=\): session must be a GenerateSession"):
            _generate(session=other)
    # the defaults are today's call: nothing of the above is looked at
    for kw in (dict(), dict(use_cache=False), dict(num_beams=3), dict(kv_cache="fp8"), dict(session=None, return_session=False)):
        with pytest.raises(_PastTheChecks):
            _generate(**kw)
    # the existing refusals come first, with their text
    with pytest.raises(ValueError, match="num_beams must be"):
        _generate(return_session=True, num_beams=0)


def test_the_engine_refuses_a_chunk_outside_a_plain_continued_prefill():
    ck, pos, _, _, t_off = eng.chunk_layout([3, 5], [2, 1])
    x = torch.zeros(6, 8)
    w = [None] * 9
    t_dev = torch.zeros(1, dtype=torch.int32)
    cache = torch.zeros(2, 16, 16)
    for kw in (dict(t_dev=t_dev), dict(kv8=torch.zeros(2, 16, 4)), dict(beam=eng.Beam(None, 2, 3)), dict(spec=eng.Spec(None, 3))):
        with pytest.raises(ValueError, match="Chunk takes the B \\* Sc new rows of a continued prefill"):
            eng.llama_layer_cached(x, 2, 3, 0, cache, 16, pos, None, None, 2, 1e-6, *w, ragged=ck, **kw)
    with pytest.raises(ValueError):                               # Sn is not the chunk's Sc
        eng.llama_layer_cached(x, 2, 2, 0, cache, 16, pos, None, None, 2, 1e-6, *w, ragged=ck)
    with pytest.raises(ValueError):                               # a SharedPrompt in place of the cache
        eng.llama_layer_cached(x, 2, 3, 0, eng.SharedPrompt(cache, cache, 1, 16), 16, pos, None, None, 2, 1e-6, *w, ragged=ck)


# ---------------------------------------------------------------------------------------------- bookkeeping --
EOS, PAD = 2, 0


def test_the_final_token_by_eos_by_stop_sequence_and_by_max_new_tokens():
    f = Mo._session_final
    assert f([7, 8, EOS, PAD, PAD], EOS, None) == 3                     # its eos; the pads behind it never count
    assert f([EOS, PAD, PAD], EOS, None) == 1
    assert f([7, 8, 9, 10], EOS, None) == 4                             # max_new_tokens: its last token
    assert f([7, 8, 9, 10], None, None) == 4
    assert f([7, 4, 5, PAD], EOS, [[4, 5]]) == 3                        # the last id of the stop sequence that ended it
    assert f([4, 5, 4, 5], EOS, [[9], [5, 4]]) == 3
    assert f([5, 4, 5, 9], EOS, [[4, 5, 9]]) == 4
    assert f([4, 5], EOS, [[3, 4, 5]]) == 2                             # the window never reaches in front of the call
    assert f([7, EOS, 4, 5], EOS, [[4, 5]]) == 2 and f([4, 5, EOS], EOS, [[4, 5]]) == 2      # whichever comes first
    assert f([PAD, PAD, 3], EOS, None) == 3                             # a generated id equal to pad is a token like any
    # pad == eos (generate's default pad): the first of them ends the sample
    assert f([7, 2, 2, 2], 2, None) == 2


def test_the_books_of_a_first_and_of_a_continued_turn():
    # first turn: valid prompt tokens n = [4, 2, 3]; rows as generate returned them (width 5)
    rows = [[7, 8, EOS, PAD, PAD], [9, 9, 9, 9, 9], [6, 4, 5, PAD, PAD]]
    cached, pending, added = Mo.GenerateSession.book([4, 2, 3], [[1, 11, 12, 13], [1, 21], [1, 31, 32]], rows, EOS, [[4, 5]])
    assert cached == [4 + 3 - 1, 2 + 5 - 1, 3 + 3 - 1] and pending == [EOS, 9, 5]
    assert added == [[1, 11, 12, 13, 7, 8, EOS], [1, 21, 9, 9, 9, 9, 9], [1, 31, 32, 6, 4, 5]]
    s = Mo.GenerateSession([torch.zeros(3, 16, 8, dtype=torch.bfloat16)], cached, torch.tensor(pending), added, 4,
                           torch.device("cpu"))
    assert s.batch == 3 and s.lengths == [7, 7, 6] and s.capacity == 16 and s.turns == 1
    assert s.ids == added and [len(r) for r in s.ids] == s.lengths
    s.ids[0].append(99)                                                 # read-only: a copy
    assert s.ids == added
    # second turn: v = [2, 1, 3] valid new tokens -> the chunk's k_len = cached + 1 + v; embeddings only
    ck = eng.chunk_layout(s._cached_host, [2, 1, 3])[0]
    assert list(ck.k_host) == [9, 8, 9]
    rows2 = [[5, 5], [EOS, PAD], [8, EOS]]
    books = Mo.GenerateSession.book(ck.k_host, None, rows2, EOS, None)
    assert books[0] == [9 + 2 - 1, 8 + 1 - 1, 9 + 2 - 1] and books[1] == [5, EOS, EOS]
    assert books[2] == [[5, 5], [EOS], [8, EOS]]                        # embeddings: the generated tokens only
    s._advance(*books)
    assert s.turns == 2 and s.lengths == [11, 9, 11] and s._cached.tolist() == [10, 8, 10] and s._pending.tolist() == [5, EOS, EOS]
    assert s.ids[1] == [1, 21, 9, 9, 9, 9, 9, EOS]
    # the history's length is the fed tokens + the pending one, whatever the known ids are
    assert [len(r) for r in s.ids] == [9, 8, 8]
