"""Drop-in mirror of the reference's `modeling.py` surface on the MI355X-native engine.

Same class names, constructor kwargs, attribute names and state-dict keys as
/root/reference/modeling.py (MM_LLMs_Config :807-861, MM_LLMs :863-1093, the vendored
LLaMA classes :44-659), so `from modeling import MM_LLMs, MM_LLMs_Config` in
run_clm_llms.py:95 / llm_trainer.py:114 keeps working (a `modeling.py` shim at the repo root
re-exports this module).  Every arithmetic op of forward and backward runs in the
hand-written gfx950 kernels of csrc/ through macaw_llm_amd.engine; there is no eager
fallback — calling the model on CPU tensors raises MacawHipError.

The CLIP / Whisper towers are instantiated from the installed `transformers` classes purely
as PARAMETER CONTAINERS (identical module tree => identical checkpoint keys, including the
never-used text tower / decoder); their HF `forward` is never called.
"""
from __future__ import annotations

import collections
import copy
import math
import numbers
import os
from typing import List, Optional, Tuple, Union

import numpy as np
import torch
from torch import nn
from torch.nn import CrossEntropyLoss
from transformers import (CLIPConfig, CLIPModel, LlamaConfig, PretrainedConfig, PreTrainedModel,
                          WhisperConfig, WhisperModel)
from transformers.modeling_outputs import BaseModelOutputWithPast, CausalLMOutputWithPast

from . import engine as eng
from . import ops
from .lib import MacawHipError


def _dev_check(t: torch.Tensor):
    if not t.is_cuda:
        raise MacawHipError("macaw_llm_amd runs on the HIP device only (model and inputs must be on "
                            "'cuda'); there is no CPU path")


def _dtype_check(dtype):
    """bf16, fp16 (the reference's scripts: train.sh `--fp16 True`, llm_trainer.py:411-412
    `.to(torch.float16)`) and fp32 (parity mode) parameters are implemented: the same kernels
    instantiated per element type (csrc/common.h E16<>), fp32 accumulation everywhere."""
    if dtype not in (torch.bfloat16, torch.float16, torch.float32):
        raise MacawHipError(f"macaw_llm_amd: model parameters are {dtype}; the gfx950 kernels implement bfloat16, "
                            "float16 and float32")


# Parameters that feed one GEMM (q|k|v, gate|up) are re-homed back to back in ONE buffer the first
# time a layer runs on the device (and again after .to() / .cuda() / any re-materialisation gave
# them separate storage), so a model built the reference's way -- MM_LLMs(config), .to(), Trainer --
# runs the same fused GEMMs as factory.build_model.  MACAW_NO_AUTO_FUSE=1 disables it.
AUTO_FUSE = os.environ.get("MACAW_NO_AUTO_FUSE") is None
# MM_LLMs.set_decode_weights: the decode_weights MM_LLMs.forward hands to generate() (None, "fp8" or "mxfp4")
DECODE_WEIGHTS = [None]
# MM_LLMs.set_kv_cache: the kv_cache MM_LLMs.forward hands to generate() (None or "fp8")
KV_CACHE = [None]
# MM_LLMs.set_sampling: the sampling arguments MM_LLMs.forward hands to generate()
SAMPLING = [dict(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=None)]
# MM_LLMs.set_sampling's four warpers behind top-p, in a store of their own (HF's defaults: all off)
_WARPERS_OFF = dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
SAMPLING_WARPERS = [dict(min_p=None, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)]
# MM_LLMs.set_beam_search: the beam arguments MM_LLMs.forward hands to generate()
BEAM_SEARCH = [dict(num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1)]
# MM_LLMs.set_logits_processors: the logits processors MM_LLMs.forward hands to generate()
PROCESSORS = [dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0)]
# MM_LLMs.set_prompt_lookup: the prompt-lookup arguments MM_LLMs.forward hands to generate() (None = off)
PROMPT_LOOKUP = [dict(prompt_lookup_num_tokens=None, max_matching_ngram_size=2)]
# MM_LLMs.set_generate_mask: whether MM_LLMs.forward hands its extended attention mask to generate()
GENERATE_MASK = [False]
# MM_LLMs.set_logprobs: the log-probability arguments MM_LLMs.forward hands to generate() (only when on)
LOGPROBS = [dict(return_logprobs=False, top_logprobs=0)]
# MM_LLMs.set_guidance: the guidance_scale MM_LLMs.forward hands to generate() next to the text-only negative prompt
# (1.0 = off: forward makes the call without them)
GUIDANCE = [1.0]
# MM_LLMs.set_stopping: the stop_sequences and bad_words_ids MM_LLMs.forward hands to generate() (only when one is set)
STOPPING = [dict(stop_sequences=None, bad_words_ids=None)]
# MM_LLMs.set_parallel_samples: the num_samples MM_LLMs.forward hands to generate() (1 = off: the call without it)
PARALLEL_SAMPLES = [1]
# MM_LLMs.set_session: whether MM_LLMs.forward asks generate() for the call's GenerateSession (return_session=True)
SESSION = [False]
# MM_LLMs.set_adapters: the adapter_names MM_LLMs.forward hands to generate() (None = off: the call without them)
ADAPTERS = [None]
# MM_LLMs.set_grammar: the grammar MM_LLMs.forward hands to generate() (None = off: the call without it)
GRAMMAR = [None]
# MM_LLMs.set_penalties: the frequency_penalty, presence_penalty and logit_bias MM_LLMs.forward hands to generate() (only
# when one is set)
PENALTIES = [dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None)]
# MM_LLMs.set_sampling_params: the sampling_params MM_LLMs.forward hands to generate() (None = off: the call without them)
SAMPLING_PARAMS = [None]

# what generate(return_logprobs=True) returns: ids as without it, logprobs f32 [B, width], top_ids int64 [B, width, n] and
# top_logprobs f32 [B, width, n] (both None for top_logprobs=0)
GenerateLogprobs = collections.namedtuple("GenerateLogprobs", ["ids", "logprobs", "top_ids", "top_logprobs"])
# what LlamaForCausalLM.score returns
ScoreResult = collections.namedtuple("ScoreResult", ["token_logprobs", "lengths", "sums", "top_ids", "top_logprobs"])
# rows x vocabulary elements of one logits buffer of score(): the fed rows go through the final norm and the lm_head in
# chunks of max(1, SCORE_LOGITS_ELEMS // V) rows (2^26 elements = 128 MiB in 16 bits: 2097 rows at V = 32000)
SCORE_LOGITS_ELEMS = 1 << 26


from .beam import beam_check, beam_result  # noqa: E402


def _sampling_check(where, temperature, top_k, top_p):
    """the sampling arguments of generate(do_sample=True) / set_sampling -> (temperature, top_k with 0 = off, top_p)"""
    if not (isinstance(temperature, numbers.Real) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"{where}: temperature must be a finite number > 0, got {temperature!r}")
    if not (isinstance(top_p, numbers.Real) and 0 < top_p <= 1):
        raise ValueError(f"{where}: top_p must lie in (0, 1], got {top_p!r}")
    top_k = 0 if top_k is None else top_k
    if not isinstance(top_k, numbers.Integral) or top_k < 0:
        raise ValueError(f"{where}: top_k must be None or an integer >= 0, got {top_k!r}")
    return float(temperature), int(top_k), float(top_p)


def _warpers_check(where, min_p, typical_p, epsilon_cutoff, eta_cutoff):
    """the four warpers behind top-p of generate(do_sample=True) / set_sampling -> (min_p, typical_p, epsilon_cutoff,
    eta_cutoff) as floats, or () when all four are off (None or 0, 1, 0, 0)"""
    def real(v):
        return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v)
    min_p = 0.0 if min_p is None else min_p
    if not (real(min_p) and 0 <= min_p <= 1):
        raise ValueError(f"{where}: min_p must be None or lie in [0, 1], got {min_p!r}")
    if not (real(typical_p) and 0 < typical_p <= 1):
        raise ValueError(f"{where}: typical_p must lie in (0, 1], got {typical_p!r}")
    for name, v in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        if not (real(v) and 0 <= v < 1):
            raise ValueError(f"{where}: {name} must lie in [0, 1), got {v!r}")
    warp = (float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff))
    return () if warp == (0.0, 1.0, 0.0, 0.0) else warp


# the keys of one entry of generate(sampling_params=[...]) and what a missing one takes: generate()'s own defaults
_SAMPLING_PARAMS_DEFAULTS = dict(temperature=1.0, top_k=50, top_p=1.0, min_p=None, typical_p=1.0, epsilon_cutoff=0.0,
                                 eta_cutoff=0.0, seed=None)


def _sampling_params_check(where, params, B=None):
    """generate(sampling_params=) / set_sampling_params -> a list with one entry per prompt: None for a greedy prompt (an
    entry None, or temperature == 0: OpenAI's and vLLM's rule; its other keys are validated all the same), else a dict of
    temperature, top_k (0 = off), top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff as _sampling_check and
    _warpers_check return them, and seed (an int, or None: to be drawn).  B (None: not known yet) is the number of
    prompts the list must match; a ValueError names the entry and what is wrong with it"""
    if not isinstance(params, (list, tuple)):
        raise ValueError(f"{where}: sampling_params must be None or a list with one dict or None per prompt, got "
                         f"{type(params).__name__}")
    if B is not None and len(params) != B:
        raise ValueError(f"{where}: sampling_params holds {len(params)} entries for {B} prompts (one dict or None per "
                         "prompt)")
    rows = []
    for i, e in enumerate(params):
        at = f"{where}: sampling_params[{i}]"
        if e is None:
            rows.append(None)
            continue
        if not isinstance(e, dict):
            raise ValueError(f"{at} must be None or a dict, got {type(e).__name__}")
        unknown = [k for k in e if k not in _SAMPLING_PARAMS_DEFAULTS]
        if unknown:
            raise ValueError(f"{at}: unknown key {unknown[0]!r}; the keys are {', '.join(_SAMPLING_PARAMS_DEFAULTS)}")
        v = {**_SAMPLING_PARAMS_DEFAULTS, **e}
        t = v["temperature"]
        greedy = isinstance(t, numbers.Real) and not isinstance(t, bool) and t == 0
        t, k, p = _sampling_check(at, 1.0 if greedy else t, v["top_k"], v["top_p"])
        w = _warpers_check(at, v["min_p"], v["typical_p"], v["epsilon_cutoff"], v["eta_cutoff"]) or (0.0, 1.0, 0.0, 0.0)
        seed = v["seed"]
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
            raise ValueError(f"{at}: seed must be None or an integer, got {seed!r}")
        rows.append(None if greedy else dict(temperature=t, top_k=k, top_p=p, min_p=w[0], typical_p=w[1],
                                             epsilon_cutoff=w[2], eta_cutoff=w[3],
                                             seed=None if seed is None else int(seed)))
    return rows


def _sampling_params_rows(rows, n=1):
    """the checked entries of _sampling_params_check -> the records of ops.SampleTable for the B * n decoded rows: row
    b * n + j carries prompt b's values with stream = j.  A sampled prompt without a seed draws a 63-bit one from torch's
    default CPU generator, in prompt order (torch.manual_seed governs them)"""
    out = []
    for r in rows:
        if r is not None and r["seed"] is None:
            r = dict(r, seed=int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)))
        if r is not None:         # (top_k at or above the vocabulary is off: the record's field is an int32)
            r = dict(r, top_k=min(r["top_k"], 2 ** 31 - 1))
        out += [None if r is None else dict(r, stream=j) for j in range(n)]
    return out


MAX_LOGIT_BIAS = 1024         # entries per row of logit_bias (ops.MAX_BIAS)
_PENALTIES_OFF = dict(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None)


def _penalties_check(where, frequency_penalty, presence_penalty, logit_bias, B=None, V=None):
    """the penalty arguments of generate() / set_penalties -> None when nothing is on, else (f, p, bias): f and p lists
    of one float per prompt (None: all zeros), bias a list of one dict | None per prompt (None: no entry anywhere).
    B (None: not known yet) is the number of prompts a per-prompt form must match, V (None: not known yet) the vocabulary
    size the ids stay below; a ValueError names what is wrong"""
    def per_prompt(name, v):
        if isinstance(v, torch.Tensor):
            if v.dim() > 1:
                raise ValueError(f"{where}: {name} must be a float or one float per prompt, got a tensor {tuple(v.shape)}")
            v = v.detach().cpu().tolist()
        vals = list(v) if isinstance(v, (list, tuple)) else [v]
        for x in vals:
            if not (isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x) and -2 <= x <= 2):
                raise ValueError(f"{where}: {name} must be finite and in [-2, 2] (a float, or one per prompt), got {x!r}")
        if isinstance(v, (list, tuple)):
            if B is not None and len(vals) != B:
                raise ValueError(f"{where}: {name} holds {len(vals)} values for {B} prompts (one per prompt)")
            vals = [float(x) for x in vals]
        elif B is not None:
            vals = [float(v)] * B
        return vals if any(x != 0 for x in vals) else None

    f, p = per_prompt("frequency_penalty", frequency_penalty), per_prompt("presence_penalty", presence_penalty)
    bias = None
    if logit_bias is not None:
        rows = logit_bias
        if isinstance(rows, dict):
            rows = [rows] * (B or 1)
        elif isinstance(rows, (list, tuple)):
            if B is not None and len(rows) != B:
                raise ValueError(f"{where}: logit_bias holds {len(rows)} entries for {B} prompts (one dict or None per "
                                 "prompt)")
        else:
            raise ValueError(f"{where}: logit_bias must be None, a dict {{token id: bias}} or a list with one dict or None "
                             f"per prompt, got {type(rows).__name__}")
        for r in rows:
            if r is None:
                continue
            if not isinstance(r, dict):
                raise ValueError(f"{where}: logit_bias: every row must be a dict {{token id: bias}} or None, got "
                                 f"{type(r).__name__}")
            if len(r) > MAX_LOGIT_BIAS:
                raise ValueError(f"{where}: logit_bias: {len(r)} entries in one row; at most {MAX_LOGIT_BIAS}")
            for c, v in r.items():
                if isinstance(c, bool) or not isinstance(c, numbers.Integral) or c < 0 or (V is not None and c >= V):
                    raise ValueError(f"{where}: logit_bias: token id {c!r} is not an integer in [0, "
                                     f"{'V' if V is None else V})")
                if not (isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(v) and -100 <= v <= 100):
                    raise ValueError(f"{where}: logit_bias[{c}] must be finite and in [-100, 100], got {v!r}")
        if any(rows):
            bias = [dict(r) if r else None for r in rows]
    return None if f is None and p is None and bias is None else (f, p, bias)


def _processors_check(where, repetition_penalty, no_repeat_ngram_size, min_new_tokens):
    """the logits-processor arguments of generate() / set_logits_processors -> (repetition_penalty, no_repeat_ngram_size,
    min_new_tokens), or None when all three are off (1.0, 0, 0)"""
    if not (isinstance(repetition_penalty, numbers.Real) and not isinstance(repetition_penalty, bool)
            and math.isfinite(repetition_penalty) and repetition_penalty > 0):
        raise ValueError(f"{where}: repetition_penalty must be a finite number > 0, got {repetition_penalty!r}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_new_tokens", min_new_tokens)):
        if not isinstance(v, numbers.Integral) or isinstance(v, bool) or v < 0:
            raise ValueError(f"{where}: {name} must be an integer >= 0, got {v!r}")
    proc = (float(repetition_penalty), int(no_repeat_ngram_size), int(min_new_tokens))
    return None if proc == (1.0, 0, 0) else proc


MAX_LOOKUP_TOKENS = 15    # Q = G + 1 <= 16 rows per sample (ops.SPEC_MAX_Q)


def _lookup_check(where, num_tokens, max_matching_ngram_size):
    """the prompt-lookup arguments of generate() / set_prompt_lookup -> G, the draft tokens per step (0 = off: None or 0)"""
    if num_tokens is None:
        return 0
    if isinstance(num_tokens, bool) or not isinstance(num_tokens, numbers.Integral) or not 0 <= num_tokens <= MAX_LOOKUP_TOKENS:
        raise ValueError(f"{where}: prompt_lookup_num_tokens must be None or an integer in [0, {MAX_LOOKUP_TOKENS}] (0 = off), "
                         f"got {num_tokens!r}")
    n = max_matching_ngram_size
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 1:
        raise ValueError(f"{where}: max_matching_ngram_size must be an integer >= 1, got {n!r}")
    return int(num_tokens)


def _logprobs_check(where, return_logprobs, top_logprobs, num_beams=1, lookup=0):
    """the log-probability arguments of generate() / set_logprobs -> n, the top columns per token (0: the selected
    token's value alone), or None when they are off (False, 0)"""
    n = top_logprobs
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 0 <= n <= ops.MAX_TOP_LOGPROBS:
        raise ValueError(f"{where}: top_logprobs must be an integer in [0, {ops.MAX_TOP_LOGPROBS}], got {n!r}")
    if n > 0 and not return_logprobs:
        raise ValueError(f"{where}: top_logprobs={n} without return_logprobs=True (the top columns come back with the "
                         "log-probabilities)")
    if not return_logprobs:
        return None
    if num_beams > 1:
        raise ValueError(f"{where}(return_logprobs=True) with num_beams={num_beams}: per-token log-probabilities along "
                         "back-tracked beams are not built; return_beam_scores=True gives each hypothesis' score")
    if lookup:
        raise ValueError(f"{where}(return_logprobs=True) with prompt_lookup_num_tokens={lookup}: a verify step emits "
                         "several tokens per launch; log-probabilities behind it are not built")
    return int(n)


def _stopping_check(where, stop_sequences, bad_words_ids, eos=None, num_beams=1, lookup=0):
    """the token-sequence arguments of generate() / set_stopping -> (stop, bad): each a list of lists of ints, or None when
    it is off.  A bad word equal to [eos] is dropped (HF's rule); none left: off"""
    got = []
    for name, v in (("stop_sequences", stop_sequences), ("bad_words_ids", bad_words_ids)):
        if v is None:
            got.append(None)
            continue
        shown = repr(v) if len(repr(v)) <= 120 else repr(v)[:117] + "..."
        if not isinstance(v, list) or len(v) == 0 or any(not isinstance(q, list) or len(q) == 0 for q in v):
            raise ValueError(f"{where}: {name} must be None or a non-empty list of non-empty lists of token ids, got {shown}")
        if any(isinstance(c, bool) or not isinstance(c, numbers.Integral) or c < 0 for q in v for c in q):
            raise ValueError(f"{where}: {name} must hold integer token ids >= 0, got {shown}")
        if len(v) > ops.MAX_SEQS:
            raise ValueError(f"{where}: {name} holds {len(v)} sequences; at most {ops.MAX_SEQS} are built")
        long = max(len(q) for q in v)
        if long > ops.MAX_SEQ_LEN:
            raise ValueError(f"{where}: {name} holds a sequence of {long} ids; at most {ops.MAX_SEQ_LEN} are built")
        if num_beams > 1:
            raise ValueError(f"{where}({name}=) with num_beams={num_beams}: matching along each beam's back-tracked history "
                             "is not built; use num_beams=1")
        if lookup:
            raise ValueError(f"{where}({name}=) with prompt_lookup_num_tokens={lookup}: matching inside a multi-token verify "
                             "step is not built")
        got.append([[int(c) for c in q] for q in v])
    stop, bad = got
    if bad is not None:
        bad = [q for q in bad if q != [eos]] or None
    return stop, bad


def _grammar_check(where, grammar, num_beams=1, lookup=0, session=False):
    """the grammar of generate() / set_grammar -> a TokenDFA (every row) or a list of TokenDFA | None (one per prompt)"""
    from .grammar import TokenDFA
    rows = list(grammar) if isinstance(grammar, (list, tuple)) else [grammar]
    for g in rows:
        if not isinstance(g, TokenDFA) and not (g is None and isinstance(grammar, (list, tuple))):
            raise ValueError(f"{where}: grammar must be None, a grammar.TokenDFA or a list of TokenDFA | None (one per "
                             f"prompt), got {type(g).__name__}")
    if isinstance(grammar, (list, tuple)) and not rows:
        raise ValueError(f"{where}: grammar is an empty list; pass None, a grammar.TokenDFA or one entry per prompt")
    if num_beams > 1:
        raise ValueError(f"{where}(grammar=) with num_beams={num_beams}: grammars along each beam's back-tracked history "
                         "are not built; use num_beams=1")
    if lookup:
        raise ValueError(f"{where}(grammar=) with prompt_lookup_num_tokens={lookup}: a constrained multi-token verify step "
                         "is not built")
    if session:
        raise ValueError(f"{where}(grammar=) with session= / return_session=True: a grammar's state is not kept across "
                         "sessions (not built)")
    return rows if isinstance(grammar, (list, tuple)) else grammar


def _grammar_rows(gram, n_prompts, V):
    """generate(grammar=) once the batch and the vocabulary are known -> one TokenDFA | None per prompt"""
    rows = gram if isinstance(gram, list) else [gram] * n_prompts
    if len(rows) != n_prompts:
        raise ValueError(f"generate(grammar=): a list of {len(rows)} grammars for {n_prompts} prompts (one per prompt, None "
                         "for an unconstrained row)")
    for g in rows:
        if g is not None and g.vocab_size is not None and g.vocab_size != V:
            raise ValueError(f"generate(grammar=): the grammar's vocabulary size {g.vocab_size} is not the model's ({V})")
    return rows


def _guidance_check(where, guidance_scale):
    """the guidance_scale of generate() / set_guidance -> the scale, or None when guidance is off (None or 1)"""
    s = guidance_scale
    if s is None:
        return None
    if isinstance(s, bool) or not isinstance(s, numbers.Real) or not math.isfinite(s):
        raise ValueError(f"{where}: guidance_scale must be None or a finite number (1 = off), got {s!r}")
    return None if s == 1 else float(s)


def _num_samples_check(where, num_samples):
    """the num_samples of generate() / set_parallel_samples -> n, the samples drawn per prompt (1 = off)"""
    n = num_samples
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or not 1 <= n <= ops.SHARED_MAX_N:
        raise ValueError(f"{where}: num_samples must be an integer in [1, {ops.SHARED_MAX_N}], got {n!r}")
    return int(n)


def _guided_batch(scale, emb, mask, neg, neg_mask):
    """The token rows of generate(guidance_scale=): the B prompts emb [B, Sc, D] (mask [B, Sc] or None = ones) on top of
    their negative prompts neg [B, Sn, D] (neg_mask or None = ones), both padded at the right to the longer length ->
    (embeddings [2B, S, D], key mask [2B, S] with a zero on every pad row).  ValueError for a negative batch, hidden size,
    dtype or mask shape that does not match"""
    B, Sc, D = emb.shape
    what = f"generate(guidance_scale={scale!r})"
    if neg.dim() != 3 or neg.shape[0] != B or neg.shape[2] != D or neg.shape[1] < 1:
        raise ValueError(f"{what}: the negative prompt should be [{B}, Sn >= 1, {D}] like the prompt's {tuple(emb.shape)}, "
                         f"but is {tuple(neg.shape)}")
    if neg.dtype != emb.dtype:
        raise ValueError(f"{what}: the negative prompt is {neg.dtype}, the prompt {emb.dtype}")
    Sn = neg.shape[1]
    if mask is not None and (mask.dim() != 2 or tuple(mask.shape) != (B, Sc)):
        raise ValueError(f"attention_mask should be of size {(B, Sc)}, but is {tuple(mask.shape)}")
    if neg_mask is not None and (neg_mask.dim() != 2 or tuple(neg_mask.shape) != (B, Sn)):
        raise ValueError(f"{what}: negative_prompt_attention_mask should be of size {(B, Sn)}, but is "
                         f"{tuple(neg_mask.shape)}")
    S, dev = max(Sc, Sn), emb.device
    rows = torch.zeros((2 * B, S, D), dtype=emb.dtype, device=dev)
    rows[:B, :Sc] = emb
    rows[B:, :Sn] = neg.to(dev)
    keys = torch.zeros((2 * B, S), dtype=torch.int32, device=dev)
    keys[:B, :Sc] = 1 if mask is None else (mask.to(dev) != 0)
    keys[B:, :Sn] = 1 if neg_mask is None else (neg_mask.to(dev) != 0)
    return rows, keys


# ---------------------------------------------------------------- the helpers of generate()'s decode loops -----
_16BIT = (torch.bfloat16, torch.float16)


def _session_final(row, eos, stop):
    """c: the generated tokens of one sample (row: its ids of one call, pads behind its end included) up to and including
    its FINAL token -- its eos, the last id of the stop sequence that ended it (stop: lists of ids, or None), or its last
    token when neither came.  Pads behind the final token never count."""
    for t, tok in enumerate(row):
        if eos is not None and tok == eos:
            return t + 1
        for q in stop or ():
            if t + 1 >= len(q) and list(row[t + 1 - len(q):t + 1]) == list(q):
                return t + 1
    return len(row)


class GenerateSession:
    """A multi-turn conversation of LlamaForCausalLM.generate: the KV caches of a batch kept alive between calls
    (generate(return_session=True) makes one, generate(session=s) continues it in place).

    The rule.  A sample's history is built turn by turn: the valid tokens of the turn's prompt, then the turn's generated
    tokens up to and including the sample's final token (its eos, the last id of the stop sequence that ended it, or its
    last token at max_new_tokens; pads behind it never enter).  A continued call returns for every sample what a fresh
    call would return for that sample alone on history + valid tokens of the new prompt, positions 0 ... len - 1, up to
    the last bits of its arithmetic.  The final token of a turn was emitted but never fed, so its key is not in the
    cache: it is the session's pending token and becomes row 0 of the next call's prefill.

    Read-only: batch, lengths (tokens of each sample's history), capacity (rows of the caches), turns, ids (per sample
    the KNOWN token ids of its history: a turn given as embeddings contributes its generated tokens only)."""

    def __init__(self, kvc, cached, pending, ids, hidden, dev):
        self._kvc = list(kvc)                    # per layer [B, capacity, 2D]: the compacted [keys | values] rows
        self._cached_host = [int(c) for c in cached]       # rows of each sample's cache = lengths - 1
        self._cached = torch.tensor(self._cached_host, dtype=torch.int32, device=dev)
        self._pending = pending.to(dev).long().contiguous()     # int64 [B]: each sample's final token, not yet fed
        self._ids = [list(r) for r in ids]
        self._hidden, self._dtype, self._device, self._turns = hidden, kvc[0].dtype, dev, 1

    batch = property(lambda self: len(self._cached_host))
    lengths = property(lambda self: [c + 1 for c in self._cached_host])
    capacity = property(lambda self: self._kvc[0].shape[1])
    turns = property(lambda self: self._turns)
    ids = property(lambda self: [list(r) for r in self._ids])

    @staticmethod
    def book(start, prompt_ids, rows, eos, stop):
        """the bookkeeping of one turn on the host, per sample: start[b] = the rows of its cache behind the turn's prefill
        (its history's length up to the prompt's last valid token), prompt_ids[b] = the prompt's valid ids (prompt_ids
        None: a turn given as embeddings), rows[b] = the ids the call returned for it, eos / stop = the call's.  With c_b
        the generated tokens up to the final token: -> (cached [B] = start + c - 1, the fed tokens; pending [B] = the
        final tokens; the known ids the turn adds [B])"""
        cached, pending, added = [], [], []
        for b, row in enumerate(rows):
            c = _session_final(row, eos, stop)
            cached.append(start[b] + c - 1)
            pending.append(int(row[c - 1]))
            added.append(([int(i) for i in prompt_ids[b]] if prompt_ids is not None else []) + [int(i) for i in row[:c]])
        return cached, pending, added

    def _advance(self, cached, pending, added):
        self._cached_host = [int(c) for c in cached]
        self._cached.copy_(torch.tensor(self._cached_host, dtype=torch.int32))
        self._pending.copy_(torch.tensor(pending, dtype=torch.long))
        for r, a in zip(self._ids, added):
            r.extend(a)
        self._turns += 1


def _session_refusal(session, return_session, use_cache, K, N, G, cfg, kv_cache):
    """generate(session=) / generate(return_session=True), stage (a): what the arguments alone refuse; None: nothing"""
    if session is None and not return_session:
        return None
    what = "generate(session=)" if session is not None else "generate(return_session=True)"
    if session is not None and not isinstance(session, GenerateSession):
        return f"{what}: session must be a GenerateSession (generate(return_session=True) returns one), got {type(session).__name__}"
    if not use_cache:
        return f"{what} with use_cache=False: a session is its KV cache"
    if K > 1:
        return f"{what} with num_beams={K}: sessions along beams are not built; use num_beams=1"
    if N > 1:
        return f"{what} with num_samples={N}: a session over parallel samples is not built; use num_samples=1"
    if G:
        return f"{what} with prompt_lookup_num_tokens={G}: a verify step over a session's ragged cache is not built"
    if cfg is not None:
        return f"{what} with guidance_scale={cfg!r}: a guided session is not built"
    if kv_cache == "fp8":
        return f"{what} with kv_cache='fp8': there is no quantised attention over several new positions"
    return None


def _no_decode_graph(decode_graph, max_new_tokens):
    """why generate() does not capture its decode step in a hipGraph; None: it does"""
    if not decode_graph:
        return "decode_graph=False selects the eager decode loop"
    if os.environ.get("MACAW_NO_DECODE_GRAPH"):
        return "MACAW_NO_DECODE_GRAPH selects the eager decode loop"
    if max_new_tokens <= 2:
        return f"max_new_tokens={max_new_tokens} <= 2: no decode step is captured"
    return None


def _attn_refusal(dtype, hd, positions, rows=None):
    """the clause that names why a step attention kernel does not take a call -- ops.decode_attn_ok, or with rows (the
    token rows per sample of a verify step) ops.spec_attn_ok; None: it does"""
    if rows is None:
        ok = ops.decode_attn_ok(dtype, hd, positions)
        what = f"ops.decode_attn_ok is false for head size {hd} and {positions} positions"
    else:
        ok = ops.spec_attn_ok(dtype, hd, positions, rows)
        what = f"ops.spec_attn_ok is false for head size {hd}, {positions} positions and {rows} rows"
    return None if ok else f"fp32 parameters ({dtype})" if dtype not in _16BIT else what


def _decode_fp8_check(dtype, hd, B, S0, max_new_tokens, use_cache, no_graph, switch="decode_weights", value="fp8", beams=1,
                      guided=False):
    """generate(decode_weights="fp8") and generate(kv_cache="fp8") run on the hipGraph decode path only: name
    what keeps a call off that path instead of decoding it in 16 bits (no_graph: _no_decode_graph's answer).  The limit
    of 32 sequences belongs to the weight-streaming step (switch="decode_weights", value "fp8" or "mxfp4"); the e4m3
    cache takes any batch.  guided: B counts the 2 x samples token rows of a call with guidance_scale."""
    why = None
    attn = _attn_refusal(dtype, hd, S0 + max_new_tokens)
    if dtype not in _16BIT:
        why = f"{attn}: the decode kernels stream bf16 / fp16 tokens"
    elif not use_cache:
        why = ("use_cache=False recomputes the prefix with the 16-bit weights" if switch == "decode_weights" else
               "use_cache=False keeps no KV cache")
    elif no_graph is not None:
        why = no_graph
    elif B * beams > 32 and switch == "decode_weights" and beams > 1:
        why = (f"B x num_beams = {B} x {beams} = {B * beams} rows: the weight-streaming decode step takes at most 32 "
               "(B * K <= 32)")
    elif B > 32 and switch == "decode_weights" and guided:
        why = (f"2 x B = 2 x {B // 2} = {B} rows under guidance_scale: the weight-streaming decode step takes at most 32 "
               "(2 B <= 32)")
    elif B > 32 and switch == "decode_weights":
        why = f"{B} sequences: the weight-streaming decode step takes at most 32"
    elif attn is not None:
        why = f"{attn}: the eager decode loop would run"
    if why is not None:
        raise ValueError(f"generate({switch}='{value}'): {why}")


def _prompt_history(input_ids, B, dev, what, ragged=None):
    """the prompt's ids as the history in front of the generated tokens -> (hist int64 [B, P], count int32 [B]).  `what`
    names the user in the refusal of another shape.  ragged (a padded batch): only the valid ids, in order, as the sample
    alone would hold them"""
    hist = input_ids.to(dev).long()
    if hist.dim() != 2 or hist.shape[0] != B:
        raise ValueError(f"generate: input_ids should be [{B}, P] as {what}, but is {tuple(hist.shape)}")
    if ragged is None:
        return hist.contiguous(), torch.full((B,), hist.shape[1], dtype=torch.int32, device=dev)
    S0 = ragged.kmask.shape[1]
    if hist.shape[1] != S0:
        raise ValueError(f"generate: input_ids should be of size {(B, S0)} next to a padded attention_mask, but is "
                         f"{tuple(hist.shape)}")
    valid = ragged.kmask != 0
    slot = torch.where(valid, ragged.slot, torch.full_like(ragged.slot, S0)).long()
    hist = torch.zeros((B, S0 + 1), dtype=torch.long, device=dev).scatter_(1, slot, hist)[:, :S0]
    return hist.contiguous(), valid.sum(1).to(torch.int32).contiguous()


def _decode_steps(step, done, n_steps, graph):
    """Run step() -- the launches of one decode step, every input and output in device memory -- until n_steps have run
    or every flag of `done` (bool, on the device) is set; returns the steps run.  graph: one step runs eagerly (it sets
    kernel attributes, allocator pools and the workspace), the next is captured in a hipGraph and replayed, and the host
    reads the flags only before those two and after every 8th replay, so up to 7 steps may run past the end (their
    emits write pad).  Otherwise the host reads the flags before every step.  Each read is a device synchronisation."""
    ran = 0
    if not graph:
        while ran < n_steps and not bool(done.all()):
            step()
            ran += 1
        return ran
    if ran < n_steps and not bool(done.all()):
        step()
        ran += 1
    if ran < n_steps and not bool(done.all()):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            step()
        for i in range(n_steps - ran):
            g.replay()
            ran += 1
            if (i & 7) == 7 and bool(done.all()):
                break
    return ran


def _step_state(S0, dev):
    """the device state of a decode loop: int32 [position fed, output column, 0, 0]"""
    return torch.tensor([S0, 0, 0, 0], dtype=torch.int32, device=dev)


class _Sampler:
    """How generate() picks a token from a row of logits, decided once behind the checks.  how: None (the argmax), the
    scalar tuple of do_sample=True -- (temperature, top_k, top_p, seed), followed by (min_p, typical_p, epsilon_cutoff,
    eta_cutoff) when one of those four is on -- or the ops.SampleTable of sampling_params.  kind: 0 the argmax, 1 the
    4-tuple, 2 the 8-tuple, 3 the table; args: what the kind's launch takes behind the common arguments"""

    def __init__(self, how):
        table = isinstance(how, ops.SampleTable)
        self.args = () if how is None else (how,) if table else tuple(how)
        self.kind = 0 if how is None else 3 if table else 1 if len(how) == 4 else 2

    def pick(self, lg, V, t):         # an eager loop: the ids [rows] of new token t
        if not self.kind:
            return ops.argmax_rows(lg, V)
        return (ops.sample_rows, ops.sample_rows_warp, ops.sample_rows_table)[self.kind - 1](lg, V, *self.args, step=t)

    def emit(self, lg, V, pad, eos, tok, done, out, state):       # the captured step: pick and bookkeeping in one launch
        fn = (ops.decode_emit, ops.decode_emit_sample, ops.decode_emit_sample_warp, ops.decode_emit_sample_table)[self.kind]
        fn(lg, V, pad, eos, tok, done, out, state, *self.args)


class _Selection:
    """What stands between the hidden rows of a step and its tokens in generate()'s greedy and sampled loops, once:

        lm_head (guidance: ops.cfg_combine of the two rows of a sample)
        -> rewrite: ops.logits_process, ops.logits_penalize, ops.seq_ban, ops.grammar_mask, in place
        -> the pick (_Sampler)
        -> flags: ops.grammar_advance (stateful: once per step), then match (ops.stop_match, stateless)
        -> the log-probabilities of the rewritten logits

    The object owns the device tables (bias, banned and stop sequences, grammar, sampling records), the per-row state
    (ids [rows, n_max]: the generated ids, pad behind a row's end -- the captured loop's output matrix, and in an eager
    loop allocated and written only where a rewrite or a flag reads it; done; the grammar's state and ends) and the prompt
    history of the processors.  rows counts what the picks see: the samples, each once under guidance (the lm_head then
    takes 2 * rows hidden rows), per_prompt of them for every entry of the per-prompt arguments pen / gram / params.

    The two steps differ in ONE place, on purpose.  captured_step runs flags in FRONT of ops.decode_emit_logprobs: that
    launch latches the done flag for the next step, and scores this step's token whatever the flag says, so the token
    that completes a stop sequence keeps its value.  eager_step looks at the flags first (a row finished BEFORE this
    step scores 0.0 / pad / 0.0), then ORs in eos, then runs flags: the same values, with the host holding the latch."""

    def __init__(self, head, emb_w, rows, V, n_max, eos, pad, dev, per_prompt=1, sample=None, params=None, n_top=None,
                 proc=None, hist=None, hist_len=None, pen=None, bad=None, stop=None, gram=None, cfg=None):
        self.head, self.emb_w, self.B, self.V, self.n_max, self.eos, self.pad, self.dev = head, emb_w, rows, V, n_max, eos, pad, dev
        self.n_top, self.proc, self.hist, self.hist_len, self.cfg = n_top, proc, hist, hist_len, cfg

        def each(v, dtype):           # one value per prompt -> one per row, on the device
            return torch.tensor(v, dtype=dtype).repeat_interleave(per_prompt).to(dev) if v is not None else None
        self.g_tab = self.g_state = self.g_end = None
        if gram is not None:
            from .grammar import combine
            self.g_tab, start = combine(gram, dev, V)
            self.g_state = each(start, torch.int32)
            self.g_end = torch.full((rows,), -1, dtype=torch.int32, device=dev)
        self.pen = None               # frequency f32 [rows], presence f32 [rows], ops.BiasTable
        if pen is not None:
            f, p, bias = pen
            self.pen = (each(f, torch.float32), each(p, torch.float32),
                        ops.BiasTable([r for r in bias for _ in range(per_prompt)], rows, V, dev) if bias is not None else None)
        # row b * n + j is prompt b's record with stream = j
        self.sampler = _Sampler(ops.SampleTable(_sampling_params_rows(params, per_prompt), dev) if params is not None else sample)
        self.bad_t = ops.SeqTable(bad, dev) if bad is not None else None
        self.stop_t = ops.SeqTable(stop, dev) if stop is not None else None
        self.reads_ids = any(v is not None for v in (proc, pen, self.bad_t, self.stop_t, self.g_tab))
        self.ids = None
        self.done = torch.zeros(rows, dtype=torch.bool, device=dev)
        self.out, self.lps = [], []   # an eager loop's ids and log-probabilities per token

    def _new_ids(self):
        return torch.full((self.B, self.n_max), self.pad, dtype=torch.long, device=self.dev)

    def logits(self, h_last):         # [rows, D] -> [rows, V]; guidance: [2 rows, D] -> a view of the lm_head's rows [0, rows)
        lg = self.head(h_last)
        return lg if self.cfg is None else ops.cfg_combine(lg, self.V, self.B, self.cfg)

    def feed(self, tok):              # the next step's token rows; guidance: both rows of a sample, two gathers into one buffer
        if self.cfg is None:
            return ops.embedding_fwd(self.emb_w, tok)
        x = torch.empty((2 * self.B, self.emb_w.shape[1]), dtype=self.emb_w.dtype, device=self.dev)
        ops.embedding_fwd(self.emb_w, tok, out=x[:self.B])
        ops.embedding_fwd(self.emb_w, tok, out=x[self.B:])
        return x

    def rewrite(self, lg, done, n_dev=None, n_add=0):     # in front of a pick, in place; generated: ids[:, :n_dev[0] + n_add]
        if self.proc is not None:
            ops.logits_process(lg, self.V, self.ids, n_dev, n_add, self.hist, self.hist_len, *self.proc, eos=self.eos)
        if self.pen is not None:      # behind the processors, on the generated ids alone
            ops.logits_penalize(lg, self.V, self.ids, n_dev, n_add, *self.pen)
        if self.bad_t is not None:    # on the processors' history
            ops.seq_ban(lg, self.V, self.ids, self.bad_t, n_dev, n_add, self.hist, self.hist_len)
        if self.g_tab is not None:    # behind all of them: the pick sees allowed columns alone
            ops.grammar_mask(lg, self.V, self.g_tab, self.g_state, done, self.eos)

    def match(self, done, n_dev=None, n_add=0):           # the stateless part of flags: run again per column for the width
        if self.stop_t is not None:
            ops.stop_match(self.ids, self.stop_t, done, n_dev, n_add)

    def flags(self, done, n_dev=None, n_add=0):           # behind a pick, as eos: the advance, ONCE per step, then the match
        if self.g_tab is not None:
            ops.grammar_advance(self.ids, self.g_tab, self.g_state, done, self.g_end, n_dev, n_add)
        self.match(done, n_dev, n_add)

    def eager_step(self, h_last, t):  # -> ids [rows] of new token t, pad where a row had finished; the flags and books behind it
        if t == 0 and self.reads_ids:
            self.ids = self._new_ids()
        done, lg = self.done, self.logits(h_last)
        self.rewrite(lg, done, n_add=t)
        ids = self.sampler.pick(lg, self.V, t)
        pads = torch.full_like(ids, self.pad)
        nxt = torch.where(done, pads, ids)
        self.out.append(nxt)
        if self.ids is not None:
            self.ids[:, t] = nxt
        if self.n_top is not None:    # 0.0 / pad / 0.0 where finished before
            lp, ti, tl = ops.token_logprobs(lg, self.V, ids, self.n_top)
            self.lps.append((torch.where(done, torch.zeros_like(lp), lp),
                             torch.where(done[:, None], pads[:, None], ti) if self.n_top else None,
                             torch.where(done[:, None], torch.zeros_like(tl), tl) if self.n_top else None))
        self.done = done | (nxt == self.eos)
        self.flags(self.done, n_add=t + 1)
        return nxt

    def finished(self):
        return bool(self.done.all())

    def eager_result(self):
        ids = torch.stack(self.out, dim=1)
        if self.n_top is None:
            return ids
        lp, top_ids, top_lp = (torch.stack(col, dim=1) if self.n_top or i == 0 else None for i, col in enumerate(zip(*self.lps)))
        return GenerateLogprobs(ids, lp, top_ids, top_lp)

    def start_captured(self, S0):     # the captured loop's books: step state, last ids, the log-probabilities' device books
        self.state, self.ids = _step_state(S0, self.dev), self._new_ids()
        self.tok = torch.zeros(self.B, dtype=torch.long, device=self.dev)
        self.ls = ops.LogprobState(self.B, self.n_max, self.n_top, self.pad, self.dev) if self.n_top is not None else None

    def captured_step(self, h_last):  # every launch reads its column from state[1] on the device: captured once, replayed
        lg, n_dev = self.logits(h_last), self.state[1:2]
        self.rewrite(lg, self.done, n_dev)
        self.sampler.emit(lg, self.V, self.pad, self.eos, self.tok, self.done, self.ids, self.state)
        self.flags(self.done, n_dev)
        if self.ls is not None:       # neither emit writes the logits: the values in front of the selection
            ops.decode_emit_logprobs(lg, self.V, self.tok, self.done, self.state, self.ls)

    def captured_result(self, n):
        """n columns ran (up to 7 past the end): trimmed to the width the eager loops return, which stop right after
        the token at which every row has finished -- by eos, a stop sequence or the grammar"""
        res = self.ids[:, :n]
        fin = (res == self.eos).cumsum(1) > 0
        if (self.stop_t is not None or self.g_tab is not None) and bool(self.done.all()):
            if self.stop_t is not None:       # every column's tail, once more
                hit = torch.zeros((n, self.B), dtype=torch.bool, device=self.dev)
                for c in range(n):
                    self.match(hit[c], n_add=c + 1)
                fin |= hit.t().cumsum(1) > 0
            if self.g_tab is not None:        # the ends were written when they happened: the advance is not run again
                cols = torch.arange(n, dtype=torch.int32, device=self.dev)
                fin |= (self.g_end >= 0)[:, None] & (cols[None, :] >= self.g_end[:, None] - 1)
        fin = fin.all(0)
        if bool(fin.any()):
            res = res[:, : int(torch.nonzero(fin)[0]) + 1]
        w, ls = res.shape[1], self.ls
        if ls is None:
            return res.clone()
        return GenerateLogprobs(res.clone(), ls.lp[:, :w].clone(), ls.top_ids[:, :w].clone() if self.n_top else None,
                                ls.top_lp[:, :w].clone() if self.n_top else None)


def _append_column(emb, emb_w, ids, src=None):
    """use_cache=False: the prefixes emb [R, S, D] grown by the embedding of the new ids [R'] -> [R', S + 1, D].  Row r
    continues row src[r] of emb (a beam continues its parent); None: row r, R' = R"""
    S, D = emb.shape[1:]
    R = ids.shape[0]
    nemb = torch.empty((R, S + 1, D), dtype=emb.dtype, device=emb.device)
    if src is None:
        ops.copy2d(emb, nemb, S, D, D, D, batch=R, s_src=S * D, s_dst=(S + 1) * D)
    else:
        nemb[:, :S] = emb.index_select(0, src)
    ops.copy2d(ops.embedding_fwd(emb_w, ids), nemb, 1, D, D, D, batch=R, s_src=D, s_dst=(S + 1) * D, dst_off=S * D)
    return nemb


def _rows_view(ts):
    """tensor [sum rows, ...] aliasing `ts` if they lie back to back in one storage, else None"""
    t0 = ts[0]
    ptr, es = t0.data_ptr(), t0.element_size()
    inner = t0[0].numel() if t0.dim() > 1 else 1
    rows = 0
    for t in ts:
        if (not t.is_contiguous() or t.data_ptr() != ptr + rows * inner * es or t.dtype != t0.dtype
                or t.shape[1:] != t0.shape[1:] or t.device != t0.device):
            return None
        rows += t.shape[0]
    try:
        return t0.data.as_strided((rows,) + tuple(t0.shape[1:]), t0.stride())
    except RuntimeError:   # not inside one storage
        return None


_PIN_WARNED = [False]


@torch.no_grad()
def _rehome_rows(ts):
    """concatenate along dim 0 into one new buffer and make every tensor a view of it.  Refused
    (returns None) for parameters that live in a BucketedStep's flat buckets: moving them would
    leave the optimizer and the collectives updating the bucket while the model computes with the
    copy (build the runtime with model= / call fuse_model() first to get the fused GEMMs)."""
    if any(ops.is_pinned(t.data) for t in ts):
        if not _PIN_WARNED[0]:
            _PIN_WARNED[0] = True
            import warnings
            warnings.warn("macaw_llm_amd: q|k|v / gate|up parameters already live in BucketedStep buckets and "
                          "were not fused; the layer runs one GEMM per projection (correct, slower).  Pass "
                          "model= to BucketedStep or call modeling.fuse_model(model) before building it.")
        return None
    fused = torch.cat([t.data for t in ts], dim=0).contiguous()
    off = 0
    for t in ts:
        t.data = fused[off:off + t.shape[0]]
        off += t.shape[0]
    return fused


def fused_encoder_qkv(attn):
    """([3E, E] weight, [3E] bias) aliasing the q/k/v projections of a HF CLIPAttention /
    WhisperAttention module (one GEMM with N = 3E instead of three).  The parameters themselves
    are re-homed (same state-dict keys), so there is no copy that could go stale when the towers
    are trained or reloaded; a missing k bias (Whisper) is a zero slot of the bias buffer.
    Returns (None, None) when fusing is off or the module is not on the device."""
    q, k, v = attn.q_proj, attn.k_proj, attn.v_proj
    ws = (q.weight, k.weight, v.weight)
    E = q.weight.shape[0]
    W3 = _rows_view(ws)
    b3 = getattr(attn, "_macaw_b3", None)
    es = q.weight.element_size()

    def bias_ok():
        if b3 is None or b3.dtype != q.weight.dtype or b3.device != q.weight.device or b3.numel() != 3 * E:
            return False
        if q.bias is None or v.bias is None:
            return False
        ok = q.bias.data_ptr() == b3.data_ptr() and v.bias.data_ptr() == b3.data_ptr() + 2 * E * es
        return ok and (k.bias is None or k.bias.data_ptr() == b3.data_ptr() + E * es)

    if W3 is not None and bias_ok():
        return W3, b3
    if not (AUTO_FUSE and q.weight.is_cuda) or q.bias is None or v.bias is None:
        return None, None
    with torch.no_grad():
        if W3 is None:
            if _rehome_rows(ws) is None:
                return None, None
            W3 = _rows_view(ws)
        if any(lin.bias is not None and ops.is_pinned(lin.bias.data) for lin in (q, k, v)):
            return None, None          # biases pinned in an optimizer bucket: keep the per-projection GEMMs
        b3 = torch.empty(3 * E, dtype=q.weight.dtype, device=q.weight.device)
        ops.fill_(b3, 0.0)
        for i, lin in enumerate((q, k, v)):
            if lin.bias is not None:
                b3[i * E:(i + 1) * E].copy_(lin.bias.data)
                lin.bias.data = b3[i * E:(i + 1) * E]
        attn._macaw_b3 = b3
    return W3, b3


def fuse_model(model):
    """fuse every q|k|v / gate|up projection of `model` NOW (decoder layers, and the CLIP / Whisper
    attention modules when they are on the device) instead of lazily at the first forward.  Call it
    -- or pass model= to bucketed.BucketedStep -- before parameters are handed to an optimizer
    runtime that re-homes them.  Idempotent."""
    for mod in model.modules():
        if isinstance(mod, LlamaDecoderLayer):
            mod.fuse_projections()
        elif (all(hasattr(mod, n) for n in ("q_proj", "k_proj", "v_proj", "out_proj"))
              and isinstance(getattr(mod, "q_proj"), nn.Linear) and mod.q_proj.weight.is_cuda):
            fused_encoder_qkv(mod)
    return model


# ---------------------------------------------------------------- LLaMA -----
class LlamaRotaryEmbedding(nn.Module):
    """modeling.py:94-123.  Tables are built once in fp32 and cast to the activation dtype."""

    def __init__(self, dim, max_position_embeddings=2048, base=10000, device=None):
        super().__init__()
        inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2).float().to(device) / dim))
        self.register_buffer("inv_freq", inv_freq)
        self.dim, self.base = dim, base
        self.max_seq_len_cached = max_position_embeddings
        self._tables = {}

    def tables(self, seq_len, dtype, device):
        if seq_len > self.max_seq_len_cached:
            self.max_seq_len_cached = seq_len
            self._tables = {}
        key = (dtype, str(device))
        if key not in self._tables:
            inv = 1.0 / (self.base ** (torch.arange(0, self.dim, 2).float() / self.dim))
            t = torch.arange(self.max_seq_len_cached, dtype=inv.dtype)
            emb = torch.cat((torch.einsum("i,j->ij", t, inv),) * 2, dim=-1)
            cos, sin = emb.cos().to(device), emb.sin().to(device)  # init-time only
            self._tables[key] = (ops.cast(cos, dtype), ops.cast(sin, dtype))
        return self._tables[key]


class LlamaRMSNorm(nn.Module):
    def __init__(self, hidden_size, eps=1e-6):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        _dev_check(hidden_states)
        return eng.RMSNormFn.apply(hidden_states, self.weight, self.variance_epsilon)


class LlamaMLP(nn.Module):
    def __init__(self, hidden_size: int, intermediate_size: int, hidden_act: str):
        super().__init__()
        if hidden_act != "silu":
            raise ValueError("LlamaMLP: only hidden_act='silu' is implemented")
        self.gate_proj = nn.Linear(hidden_size, intermediate_size, bias=False)
        self.down_proj = nn.Linear(intermediate_size, hidden_size, bias=False)
        self.up_proj = nn.Linear(hidden_size, intermediate_size, bias=False)


class LlamaAttention(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.hidden_size = config.hidden_size
        self.num_heads = config.num_attention_heads
        self.head_dim = self.hidden_size // self.num_heads
        self.max_position_embeddings = config.max_position_embeddings
        if (self.head_dim * self.num_heads) != self.hidden_size:
            raise ValueError(
                f"hidden_size must be divisible by num_heads (got `hidden_size`: {self.hidden_size}"
                f" and `num_heads`: {self.num_heads}).")
        self.q_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=False)
        self.k_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=False)
        self.v_proj = nn.Linear(self.hidden_size, self.num_heads * self.head_dim, bias=False)
        self.o_proj = nn.Linear(self.num_heads * self.head_dim, self.hidden_size, bias=False)
        self.rotary_emb = LlamaRotaryEmbedding(self.head_dim,
                                               max_position_embeddings=self.max_position_embeddings)


class LlamaDecoderLayer(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.hidden_size = config.hidden_size
        self.self_attn = LlamaAttention(config=config)
        self.mlp = LlamaMLP(hidden_size=self.hidden_size, intermediate_size=config.intermediate_size,
                            hidden_act=config.hidden_act)
        self.input_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.post_attention_layernorm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps)

    # ---- optional fused storage for q|k|v and gate|up ------------------------------------
    @torch.no_grad()
    def fuse_projections(self):
        """Re-home q/k/v (and gate/up) weights in ONE contiguous [3D, D] ([2FF, D]) buffer each;
        the nn.Linear parameters become row-slice views of it, so state-dict keys, optimizers
        and gradients are unchanged while the engine runs one GEMM instead of three (two)."""
        a, m = self.self_attn, self.mlp
        for mods in ((a.q_proj, a.k_proj, a.v_proj), (m.gate_proj, m.up_proj)):
            ws = [x.weight for x in mods]
            if _rows_view(ws) is None:
                _rehome_rows(ws)
        return self

    @staticmethod
    def _fused_view(ws):
        """[sum rows, D] tensor aliasing the parameters if they are laid out back to back"""
        return _rows_view(ws)

    def fused_weights(self):
        """(wqkv, wgu) views; fuses lazily on the device (AUTO_FUSE) so that the reference's own
        construction path -- MM_LLMs(config) -> resize_token_embeddings -> .to(dtype / device),
        run_clm_llms.py:478-497 -- gets the one-GEMM projections too."""
        a, m = self.self_attn, self.mlp
        qkv = (a.q_proj.weight, a.k_proj.weight, a.v_proj.weight)
        gu = (m.gate_proj.weight, m.up_proj.weight)
        wqkv, wgu = self._fused_view(qkv), self._fused_view(gu)
        if (wqkv is None or wgu is None) and AUTO_FUSE and qkv[0].is_cuda:
            self.fuse_projections()
            wqkv, wgu = self._fused_view(qkv), self._fused_view(gu)
        return wqkv, wgu

    def forward(self, hidden_states, kmask=None, pos=None, past_key_value=None, use_cache=False,
                recompute=False):
        """hidden_states [B,S,D]; kmask int32 [B,S] (0 = padding) or None; pos int32 [B*S];
        recompute = activation checkpointing for this layer."""
        if past_key_value is not None or use_cache:
            raise NotImplementedError("KV-cache decode goes through LlamaForCausalLM.generate")
        a, m = self.self_attn, self.mlp
        wqkv, wgu = self.fused_weights()
        cos, sin = a.rotary_emb.tables(hidden_states.shape[1], hidden_states.dtype,
                                       hidden_states.device)
        lora = ()
        st = getattr(self, "_lora_state", None)
        if st is not None:          # LoRA adapters (macaw_llm_amd/lora.py): their (A, B) follow as trailing inputs
            from .lora import layer_adapters
            ad = layer_adapters(self)
            if ad:
                cfg = st.config
                spec = eng.LoraSpec([i for i, _ in ad], cfg.scaling, cfg.lora_dropout if self.training else 0.0,
                                    st.seed, self._lora_layer)
                lora = (spec, *[t for _, lin in ad for t in (lin.lora_A.weight, lin.lora_B.weight)])
        out = eng.LlamaLayerFn.apply(
            hidden_states, kmask, pos, cos, sin, a.num_heads, self.input_layernorm.variance_epsilon,
            a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, m.gate_proj.weight,
            m.up_proj.weight, m.down_proj.weight, self.input_layernorm.weight,
            self.post_attention_layernorm.weight, wqkv, wgu, recompute, *lora)
        return (out,)


class LlamaPreTrainedModel(PreTrainedModel):
    config_class = LlamaConfig
    base_model_prefix = "model"
    supports_gradient_checkpointing = True
    _no_split_modules = ["LlamaDecoderLayer"]

    def _init_weights(self, module):
        std = self.config.initializer_range
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(mean=0.0, std=std)
            if module.padding_idx is not None:
                module.weight.data[module.padding_idx].zero_()

    def _set_gradient_checkpointing(self, module, value=False):
        if isinstance(module, LlamaModel):
            module.gradient_checkpointing = value


class LlamaModel(LlamaPreTrainedModel):
    def __init__(self, config: LlamaConfig):
        super().__init__(config)
        self.padding_idx = config.pad_token_id
        self.vocab_size = config.vocab_size
        self.embed_tokens = nn.Embedding(config.vocab_size, config.hidden_size, self.padding_idx)
        self.layers = nn.ModuleList([LlamaDecoderLayer(config) for _ in range(config.num_hidden_layers)])
        self.norm = LlamaRMSNorm(config.hidden_size, eps=config.rms_norm_eps)
        self.gradient_checkpointing = False
        self._pos_cache = {}
        self.post_init()

    def get_input_embeddings(self):
        return self.embed_tokens

    def set_input_embeddings(self, value):
        self.embed_tokens = value

    def _positions(self, B, S, device):
        key = (B, S, str(device))
        if key not in self._pos_cache:
            self._pos_cache = {key: torch.arange(S, dtype=torch.int32, device=device).repeat(B)}
        return self._pos_cache[key]

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None):
        if input_ids is not None and inputs_embeds is not None:
            raise ValueError("You cannot specify both decoder_input_ids and decoder_inputs_embeds at the same time")
        if input_ids is None and inputs_embeds is None:
            raise ValueError("You have to specify either decoder_input_ids or decoder_inputs_embeds")
        if output_attentions:
            raise NotImplementedError("output_attentions is not supported by the fused engine")
        if past_key_values is not None or use_cache:
            raise NotImplementedError("KV-cache decode goes through LlamaForCausalLM.generate")
        if inputs_embeds is None:
            _dev_check(input_ids)
            B, S = input_ids.shape
            inputs_embeds = EmbeddingFn.apply(self.embed_tokens.weight, input_ids.long().reshape(-1),
                                              self.padding_idx).view(B, S, -1)
        _dev_check(inputs_embeds)
        B, S, _ = inputs_embeds.shape
        dev = inputs_embeds.device
        if position_ids is None:  # modeling.py:434-439: arange(S) irrespective of padding
            pos = self._positions(B, S, dev)
        else:
            pos = position_ids.to(torch.int32).expand(B, S).reshape(-1).contiguous()
        kmask = None
        if attention_mask is not None:
            if attention_mask.shape != (B, S):
                raise ValueError(f"Attention mask should be of size {(B, S)}, but is {tuple(attention_mask.shape)}")
            kmask = attention_mask.to(torch.int32).contiguous()
        h = inputs_embeds
        all_h = () if output_hidden_states else None
        for layer in self.layers:
            if output_hidden_states:
                all_h += (h,)
            # modeling.py:474-489: checkpoint every decoder layer when training with the flag on
            h = layer(h, kmask=kmask, pos=pos,
                      recompute=self.gradient_checkpointing and self.training)[0]
        # NOTE: the final RMSNorm is fused with lm_head in LlamaForCausalLM; standalone
        # LlamaModel.forward applies it here.
        if getattr(self, "_defer_final_norm", False):
            return h
        h = self.norm(h)
        if output_hidden_states:
            all_h += (h,)
        return BaseModelOutputWithPast(last_hidden_state=h, past_key_values=None, hidden_states=all_h,
                                       attentions=None)


class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, ids, padding_idx):
        out = ops.embedding_fwd(table, ids)
        ctx.save_for_backward(ids)
        ctx.shape, ctx.padding_idx = table.shape, padding_idx
        ctx.dtype = table.dtype
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        dt = torch.empty(ctx.shape, dtype=ctx.dtype, device=dout.device)
        ops.fill_(dt, 0.0)
        ops.embedding_bwd_(dt, dout.contiguous(), ids,
                           -1 if ctx.padding_idx is None else ctx.padding_idx)
        return dt, None, None


class LlamaForCausalLM(LlamaPreTrainedModel):
    def __init__(self, config):
        super().__init__(config)
        self.model = LlamaModel(config)
        self.lm_head = nn.Linear(config.hidden_size, config.vocab_size, bias=False)
        self.post_init()

    def get_input_embeddings(self):
        return self.model.embed_tokens

    def set_input_embeddings(self, value):
        self.model.embed_tokens = value

    def get_output_embeddings(self):
        return self.lm_head

    def set_output_embeddings(self, new_embeddings):
        self.lm_head = new_embeddings

    def set_decoder(self, decoder):
        self.model = decoder

    def get_decoder(self):
        return self.model

    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None,
                inputs_embeds=None, labels=None, use_cache=None, output_attentions=None,
                output_hidden_states=None, return_dict=None):
        st = getattr(self, "_lora", None)
        if st is not None:
            st.begin_step(self.training)
        self.model._defer_final_norm = True
        try:
            h = self.model(input_ids=input_ids, attention_mask=attention_mask,
                           position_ids=position_ids, past_key_values=past_key_values,
                           inputs_embeds=inputs_embeds, use_cache=use_cache,
                           output_attentions=output_attentions)
        finally:
            self.model._defer_final_norm = False
        shift = None
        if labels is not None:
            # Shift so that tokens < n predict n (modeling.py:601-603): row (b,s) is scored
            # against labels[b, s+1]; the last position of every sample is ignored.
            labels = labels.to(h.device).long()
            shift = torch.cat([labels[:, 1:], torch.full_like(labels[:, :1], -100)], dim=1)
            shift = shift.reshape(-1).contiguous()
        loss, logits = eng.LMHeadLossFn.apply(h, self.model.norm.weight, self.lm_head.weight, shift,
                                              self.model.norm.variance_epsilon)
        loss = loss[0] if labels is not None else None
        if return_dict is False:
            return ((loss, logits) if loss is not None else (logits,))
        return CausalLMOutputWithPast(loss=loss, logits=logits, past_key_values=None,
                                      hidden_states=None, attentions=None)

    # The three decode loops on device state.  Each is its state, its emit and its step closure (the greedy / sampled
    # loop's state and emit are its _Selection's): token 0 comes from the prefill's rows, then _decode_steps runs the step
    # max_new_tokens - 1 times at the most -- with graph captured once after one eager step and replayed, the host looking
    # at the done flags every 8 steps; otherwise kernel by kernel, the host looking before every step.
    @torch.no_grad()
    def _generate_graph(self, run, chain, last, S0, max_new_tokens):
        """Decode loop with ONE hipGraph launch per token.  Everything a step needs lives in device memory -- the
        position (the int32 counter the fused RoPE + cache append + attention kernel reads), the last token ids, the
        finished flags and the output matrix, all advanced by the emit of chain (a _Selection), which also holds them --
        so the launches of a step (5 per layer + 3, and what the chain adds) are captured once, after one eager step
        that also serves as the warm-up, and replayed; the host only looks at the finished flags every few tokens."""
        chain.start_captured(S0)
        t_dev = chain.state[:1]

        def step():
            chain.captured_step(run(chain.feed(chain.tok), 1, 0, pos=t_dev, t_dev=t_dev))

        chain.captured_step(last)        # token 0 (from the prefill) ...
        chain.state[0] = S0              # ... is the one fed at position S0
        return chain.captured_result(1 + _decode_steps(step, chain.done, max_new_tokens - 1, True))

    @torch.no_grad()
    def _generate_beam(self, run, logits, last, emb_w, B, K, S0, max_new_tokens, eos, pad, dev, length_penalty,
                       early_stopping, graph):
        """The beam-search decode loop (ops.beam_emit in place of ops.decode_emit, the step's B * K rows attending through
        the indirection table): token 0 from the prefill's B rows (K_in = 1), then one step per token -- embedding of the
        K tokens per sample, the layers with engine.Beam, the lm_head, the emit.  Returns the device books and the step
        state for generate's beam_out."""
        state = _step_state(S0, dev)
        t_dev = state[:1]
        bs = ops.BeamState(B, K, max_new_tokens, pad, dev)
        beam = eng.Beam(bs.ind, K, S0)
        V = self.lm_head.weight.shape[0]

        def emit(h_last, K_in):
            ops.beam_emit(logits(h_last), V, K_in, pad, eos, length_penalty, early_stopping, bs, state)

        def step():
            emit(run(ops.embedding_fwd(emb_w, bs.tok), 1, 0, pos=t_dev, t_dev=t_dev, beam=beam), K)

        emit(last, 1)                    # token 0 (from the prefill) ...
        state[0] = S0                    # ... is the one fed at position S0
        _decode_steps(step, bs.done, max_new_tokens - 1, graph)
        return bs, state

    @torch.no_grad()
    def _generate_lookup(self, run, logits, last, emb_w, B, G, S0, max_new_tokens, eos, pad, dev, ngram, hist, hist_len,
                         graph):
        """The prompt-lookup decode loop (one VERIFY step of Q = G + 1 rows per sample in place of the one-row step):
        token 0 from the prefill's B rows through ops.spec_verify_emit (one row per sample, no draft), then per step
        ops.spec_lookup -> embedding of the [B, Q] ids -> the layers with engine.Spec -> the lm_head ->
        ops.spec_verify_emit.  Position, count and done flag live per sample on the device (ops.SpecState).  An unfinished
        sample emits at least one token per step, so max_new_tokens - 1 steps behind token 0 always suffice.  Returns (ids
        [B, most tokens of a sample], steps int32 [B])."""
        ss = ops.SpecState(B, G, max_new_tokens, pad, dev)
        ss.pos.fill_(S0 - 1)             # token 0 advances it to S0, the position its id is fed at
        spec = eng.Spec(ss.pos, G + 1)
        V = self.lm_head.weight.shape[0]

        def verify(h_rows):
            ops.spec_verify_emit(logits(h_rows), V, eos, ss)

        def step():
            ops.spec_lookup(ss, V, ngram, eos, hist, hist_len)
            verify(run(ops.embedding_fwd(emb_w, ss.tok.view(-1)), G + 1, 0, pos=ss.pos, t_dev=ss.pos, spec=spec))

        verify(last)                     # token 0 (from the prefill)
        _decode_steps(step, ss.done, max_new_tokens - 1, graph)
        width = int(ss.n_out.max())      # pad behind each sample's end; the column at which every sample has finished
        return ss.out[:, :width].clone(), ss.steps.clone()

    def _hidden_last(self, emb, mask=None, last_valid=None):
        """use_cache=False: the whole prefix emb [R, S, D] through the layers, the final norm left to the lm_head, ->
        the hidden rows [R, D] that predict the next token: the last row of every sample, or (last_valid: the flat
        indices of a padded prompt's last valid rows) those rows.  mask [R, S]: the key mask of a padded batch"""
        R, S, D = emb.shape
        self.model._defer_final_norm = True
        try:
            if mask is not None:
                h = self.model(inputs_embeds=emb, attention_mask=mask, position_ids=(mask.cumsum(1) - 1).clamp_(min=0))
            else:
                h = self.model(inputs_embeds=emb)
        finally:
            self.model._defer_final_norm = False
        if last_valid is not None:
            return ops.embedding_fwd(h.contiguous().view(R * S, D), last_valid)
        last = torch.empty((R, D), dtype=emb.dtype, device=emb.device)
        ops.copy2d(h.contiguous(), last, 1, D, D, D, batch=R, s_src=S * D, s_dst=D, src_off=(S - 1) * D)
        return last

    @torch.no_grad()
    def generate(self, inputs_embeds=None, input_ids=None, max_new_tokens=128, eos_token_id=2,
                 bos_token_id=1, pad_token_id=None, use_cache=True, decode_graph=True, decode_weights=None,
                 kv_cache=None, do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=None, min_p=None,
                 typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0, attention_mask=None, num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1,
                 return_beam_scores=False, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0,
                 prompt_lookup_num_tokens=None, max_matching_ngram_size=2, return_lookup_stats=False,
                 return_logprobs=False, top_logprobs=0, guidance_scale=None, negative_prompt_ids=None,
                 negative_prompt_attention_mask=None, negative_inputs_embeds=None, stop_sequences=None,
                 bad_words_ids=None, num_samples=1, session=None, return_session=False, session_capacity=None,
                 adapter_names=None, grammar=None, frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None,
                 sampling_params=None, **_):
        """Greedy decode by default — the only mode the reference uses (modeling.py:959:
        `llm.generate(inputs_embeds=…, max_new_tokens=128, eos_token_id=2, bos_token_id=1,
        pad_token_id=32006)`, no attention mask).  Prefill runs the prompt once and fills a
        preallocated per-layer KV cache [B, T_max, D]; every decode step runs one position
        through the layers against the cache (fused attention, Lq = 1) instead of the
        reference's per-step `torch.cat` of the cache (modeling.py:190-195).  Finished samples
        emit pad_token_id.  Returns the NEW token ids [B, <= max_new_tokens].
        use_cache=False recomputes the whole prefix each step (same ids; test reference).

        decode_weights="fp8": weight-only quantised decode (W8A16).  The decode steps and the lm_head stream
        OCP e4m3 copies of the weights, one scale per output channel (ops.fp8_weight: made once, re-made when
        the weight version moves; shared with the fp8 training configuration), through ops.decode_linear_fp8;
        tokens, KV cache and accumulation keep their precision, and the prefill keeps the 16-bit weights (a
        large-M GEMM, not a stream; the prompt's KV cache is written at full weight precision).  This is a
        LATENCY mode, not a memory one: the 16-bit masters stay resident and the copies add half their size.
        With LoRA adapters the per-call merged copies are quantised, once per call.  It needs the hipGraph
        decode path and raises ValueError naming the condition when that path would not be taken (fp32
        parameters, unfused q/k/v or gate/up storage, use_cache=False, decode_graph=False or
        MACAW_NO_DECODE_GRAPH, max_new_tokens <= 2, more than 32 sequences, a head size / length outside
        ops.decode_attn_ok) instead of silently decoding in 16 bits.  None (default): the 16-bit path.

        decode_weights="mxfp4": the same mode at 4.25 bits per weight (W4A16).  The four streamed projections of every
        layer use OCP MXFP4 copies (e2m1 codes, one power-of-two scale per 32 elements along K: ops.mxfp4_weight, cached
        and re-made like the e4m3 copies) through ops.decode_linear_mxfp4; a projection outside that kernel's domain
        (K % 128 != 0) keeps its 16-bit launch.  The lm_head streams its E4M3 copy (ops.fp8_weight): 1 % of the bytes,
        and the projection whose rounding decides the argmax.  Round-to-nearest quantisation WITHOUT calibration: the
        format error is bounded by tests/test_decode_mxfp4_gpu.py, the quality on trained checkpoints is unmeasured.
        Prefill, tokens, KV cache, accumulation, LoRA (merged copies quantised once per call) and every refusal as
        for "fp8".  Also a LATENCY mode: the 16-bit masters stay resident and the copies add 0.27 of their size.

        kv_cache="fp8": the KV cache holds OCP e4m3 bytes with one fp32 scale per (sample, position, key or value,
        head) (amax / 448 over the head's elements; keys quantised after RoPE; the format of include/macaw_hip.h):
        0.52 of the 16-bit cache's memory and of the bytes a decode step reads from it.  The query stays 16-bit,
        de-quantisation and accumulation are fp32 (ops.decode_step_attn_kv8).  The prefill attends over the prompt's
        own 16-bit keys and values and then writes the quantised cache (ops.kv_quant_append), so the first new token
        is the 16-bit path's.  The gain grows with batch x context (the weight stream of a step is fixed, the cache
        stream is not); at batch 1 and a short context the attention launch is latency-bound and the switch buys
        memory, not time (profiles/decode_kv8_generate.txt).  Composes with decode_weights="fp8".  Like that switch it
        needs the hipGraph decode path and raises ValueError naming the condition otherwise (fp32 parameters,
        use_cache=False, decode_graph=False or MACAW_NO_DECODE_GRAPH, max_new_tokens <= 2, a head size / length
        outside ops.decode_attn_ok); any batch size, fused or unfused projection storage.  None (default): the 16-bit
        cache.

        do_sample=True: sampled decoding with HF's defaults and warper order -- logits / temperature, then top_k (0 or
        None = off, as is top_k >= vocabulary), then top_p over the survivors, then one draw per sample (ops.sample_rows;
        on the hipGraph path ops.decode_emit_sample, the random number computed on the device from the output column, so
        the host still does not touch a step).  The random number of (sample b, new token t) is a counter hash of
        (seed, t, b): the same seed gives the same ids, call after call and on every decode path by itself (the paths'
        logits differ in their last bits, so ids may differ BETWEEN paths where a draw falls on a boundary).  seed=None
        draws a 63-bit seed from torch's default CPU generator (torch.manual_seed governs it); an integer is used as
        given.  One difference to HF: top_k keeps EXACTLY k columns, ties at the k-th value going to the lower column
        (HF keeps the whole tie group), which makes top_k=1 greedy.  temperature <= 0, top_p outside (0, 1] and a
        negative top_k raise ValueError.  With do_sample=False (default) the four arguments are ignored and not one
        launch differs.  Composes with decode_weights, kv_cache and LoRA (they only change where the logits come from).

        min_p, typical_p, epsilon_cutoff, eta_cutoff (do_sample=True; HF's names, defaults None, 1.0, 0.0, 0.0 = off, and
        order: behind top_p, in front of the draw; HF's MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and
        EtaLogitsWarper with min_tokens_to_keep = 1).  Each works on the survivors of the stages before it, renormalised
        over them, and keeps at least one token.  min_p in [0, 1]: a token stays iff its probability is at least min_p times
        the largest.  typical_p in (0, 1]: the tokens whose -log p lies nearest to the entropy, as many as it takes to reach
        the mass typical_p (a band around the entropy: the most likely token can go).  epsilon_cutoff in [0, 1): a token
        stays iff its probability is at least epsilon_cutoff.  eta_cutoff in [0, 1): the same with the threshold
        min(eta, sqrt(eta) * exp(-entropy)).  The rule is rule 6 next to mk_sample_rows in include/macaw_hip.h, restated
        in tests/warpers_ref.py; the stages run inside the one selection launch (csrc/sample.hip; ops.sample_rows_warp and
        ops.decode_emit_sample_warp, called in place of ops.sample_rows / ops.decode_emit_sample), so the hipGraph path
        keeps its one replay per token, and they reach every loop that samples: the eager loops, a padded batch,
        use_cache=False, guidance, num_samples, sessions, adapter_names and a grammar (they see the masked row, as top_k
        does).  Log-probabilities go on scoring the logits in front of temperature.  ops.sample_keep_rows returns the
        surviving tokens of a row of logits.  Values outside the ranges, bool, NaN and inf raise ValueError; with
        do_sample=False the four are ignored.  With all four off every launch is the one without them.

        attention_mask [B, S0] (any integer or bool dtype, non-zero = valid): a PADDED batch -- left padding, right
        padding or holes.  Sample b generates what its n_b valid tokens would generate alone, in order and unpadded:
        positions are max(cumsum(mask) - 1, 0) (the reference's LLaMA rule for such batches, modeling.py:624-652), masked
        keys are excluded, and token 0 is predicted by each sample's LAST VALID row.  The prefill runs over the padded
        rows with the key mask and writes the KV cache compacted (the valid token at position i in cache row i:
        ops.kv_append_rows / ops.kv_quant_append_rows); new token t of sample b then lives at position and cache row
        n_b + t, and the step kernels read their position per sample (ops.decode_step_attn_var / _kv8_var: the one
        device counter plus a per-sample offset), so a short sample streams only its own keys and the host still
        does nothing per token on the hipGraph path.  decode_graph=False, MACAW_NO_DECODE_GRAPH and max_new_tokens <= 2
        run the same step launches kernel by kernel.  Composes with kv_cache, decode_weights, sampling and LoRA.  A
        padded mask with use_cache=True needs those step kernels: fp32 parameters, or a head size / length outside
        ops.decode_attn_ok, raise ValueError (there is no masked attention over a cache) -- use use_cache=False, which
        recomputes the prefix with the growing mask and works for every dtype.  A sample without a valid token and a
        mask of another shape raise ValueError.  None (default) or a mask without a zero: the unpadded path, not one
        launch different.

        num_beams=K > 1: beam search with classic HF BeamSearchScorer semantics (the rule is written down in
        include/macaw_hip.h and restated in tests/beam_ref.py): K running beams per sample scored by their summed
        log-probabilities, a pool of K finished hypotheses scored sum / L ** length_penalty (L = generated tokens, the
        eos included), early_stopping=True finishing a sample once the pool holds K and False once no running beam can
        still beat its worst entry.  Returns the ids of the best num_return_sequences <= K hypotheses per sample,
        [B * num_return_sequences, longest returned hypothesis], pad_token_id behind each eos; with
        return_beam_scores=True the pair (ids, scores f32 [B * num_return_sequences]).  Every step is on the device:
        ops.beam_emit does log-softmax, the exact top-2K selection, eos, pool and done flags in one launch, and the KV
        cache [B, K, T_max, 2D] is read through a beam indirection table (ops.decode_step_attn_beam) that the emit
        updates in place -- no cache row is ever copied, the prompt's keys are stored once per sample and the prefill
        runs at batch B.  One hipGraph replay per token as for greedy; decode_graph=False, MACAW_NO_DECODE_GRAPH and
        max_new_tokens <= 2 run the same launches kernel by kernel; use_cache=False recomputes the B * K prefixes with
        the same ops.beam_emit (any dtype; test reference).  The host backtracks the (token, parent) history once,
        after the loop.  Composes with decode_weights (their limit becomes B * K <= 32) and LoRA.  ValueError naming the
        condition for num_beams outside [1, 16], num_return_sequences > num_beams, a vocabulary below 2 * num_beams,
        do_sample=True, kv_cache="fp8" and a padded attention_mask (the last two are not built), and for use_cache=True
        with fp32 parameters or a shape outside ops.decode_attn_ok (use use_cache=False).  num_beams=1 (default): today's
        path whatever the other beam arguments say, not one launch different.

        repetition_penalty, no_repeat_ngram_size, min_new_tokens: HF's logits processors of the same names, in HF's
        order and arithmetic (the rule is written down in include/macaw_hip.h and restated in tests/logits_proc_ref.py):
        every distinct id of the history has its logit divided by the penalty (multiplied when negative), in fp32 with
        one rounding to the logits' type; every id that would complete an n-gram the history already holds gets -inf;
        eos gets -inf while fewer than min_new_tokens tokens were generated.  One launch (ops.logits_process) rewrites
        the step's logits in place in front of the emit -- on the hipGraph path inside the captured step, the history
        length read from the device, so the host still does not touch a step -- and in front of the selection of the
        eager, use_cache=False and padded-batch loops; token 0 is processed too.  Sampling runs behind them
        (processors, then warpers).  The history is this call's generated tokens, with the prompt's ids in front when
        input_ids is passed (alone or next to inputs_embeds, where it is otherwise ignored; [B, P] with any P, or
        [B, S0] under a padded attention_mask, of which only the valid ids count, in order: what the sample would
        generate alone).  Embeddings alone, MM_LLMs' call, give a history of generated tokens, as in HF.  Composes with
        decode_weights, kv_cache, sampling, a padded mask and LoRA.  ValueError for a penalty that is not a finite
        number > 0, for a non-integer or negative no_repeat_ngram_size / min_new_tokens, and for any of them with
        num_beams > 1 (processors along each beam's back-tracked history are not built).  min_new_tokens needs an
        eos_token_id; a vocabulary above 2^18 is outside ops.logits_process.  With the defaults (1.0, 0, 0) not one
        launch differs.

        prompt_lookup_num_tokens=G in [1, 15]: prompt-lookup speculative decoding, HF's argument of the same name, greedy
        (the rule is written down in include/macaw_hip.h and restated in tests/spec_ref.py).  Every step proposes up to G
        draft tokens per sample -- the continuation of the earliest earlier occurrence of the history's last
        max_matching_ngram_size ids, shorter n-grams down to 1 when that one has none (ops.spec_lookup) -- and verifies
        them in ONE pass of G + 1 token rows per sample over the weights: ops.decode_step_attn_multi appends the G + 1
        keys and lets row g attend up to its own position, ops.spec_verify_emit keeps the draft tokens that equal the
        model's own argmax plus one more token.  Every emitted id is the argmax of the model's logits given the ids
        before it, as in plain greedy decoding; a step's linears see B * (G + 1) rows and choose their kernel by that, so
        last bits, and with them near-ties, may differ from the one-row step's.  The history is this call's generated
        tokens with input_ids [B, P] in front where it is given (alone or next to inputs_embeds, any P).  All state
        (position, count, done flag per sample) is on the device: one hipGraph replay per step, the host looking at the
        done flags every 8 steps; decode_graph=False, MACAW_NO_DECODE_GRAPH and max_new_tokens <= 2 run the same launches
        kernel by kernel.  The KV cache gets G more rows.  Returns the new ids [B, <= max_new_tokens], pad_token_id behind
        each sample's end; with return_lookup_stats=True the pair (ids, steps int32 [B]: verify steps per sample, token 0
        included, so tokens / steps is the gain).  Composes with decode_weights (their limit becomes B * (G + 1) <= 32)
        and LoRA.  ValueError naming the condition for G outside [0, 15] or not an integer, max_matching_ngram_size < 1,
        B * (G + 1) > 32, num_beams > 1, do_sample=True, any logits processor, kv_cache="fp8", a padded attention_mask,
        use_cache=False, fp32 parameters and a shape outside ops.spec_attn_ok: none of these combinations is built.  None
        or 0 (default): today's path, not one launch different.

        return_logprobs=True: the call returns the named tuple GenerateLogprobs(ids, logprobs, top_ids, top_logprobs) --
        ids exactly the tensor the call returns without it, logprobs f32 [B, width] the log-softmax value of every
        emitted token, and with top_logprobs=n in [1, 20] top_ids int64 [B, width, n] and top_logprobs f32 [B, width, n],
        the n most likely columns of every step in descending order, ties to the lower column (both None for n = 0).  The
        rule is written down in include/macaw_hip.h and restated in tests/logprobs_ref.py: fp64 log-sum-exp, one
        rounding to fp32; a row without a finite logit or with +inf gives NaN.  The log-probabilities are those of the
        logits as they stand in front of the selection: after the logits processors, which rewrite them in place, and
        before temperature / top-k / top-p.  For greedy decoding that is HF's compute_transition_scores(...,
        normalize_logits=True).  For sampling it is the model's unwarped distribution, NOT the renormalised one the draw
        used.  Columns behind a sample's end hold 0.0, pad_token_id and 0.0; the eos itself has its real value.  On the
        hipGraph path one more launch per step (ops.decode_emit_logprobs behind the emit, inside the captured step: still
        one replay per token, and the host reads nothing more); the eager, padded-batch and use_cache=False loops call
        ops.token_logprobs on the processed logits with the selected ids (any dtype).  Composes with decode_weights,
        kv_cache, sampling, processors, a padded mask and LoRA.  ValueError naming the condition for top_logprobs not an
        integer in [0, 20], top_logprobs > 0 without return_logprobs=True, num_beams > 1 (return_beam_scores stays what
        beams offer) and prompt_lookup_num_tokens > 0: not built.  Defaults (False, 0): nothing is allocated, launched or
        read.

        guidance_scale=s with negative_prompt_ids [B, Sn] or negative_inputs_embeds [B, Sn, D] (and optionally
        negative_prompt_attention_mask [B, Sn]): classifier-free guidance, HF's arguments of the same names
        (UnbatchedClassifierFreeGuidanceLogitsProcessor; negative_inputs_embeds is the partner of inputs_embeds).  Every
        step is scored twice, on the prompt and on the negative prompt, and decodes from
        log p_neg + s * (log p_prompt - log p_neg) (the rule is written down in include/macaw_hip.h and restated in
        tests/cfg_ref.py: fp64 log-sum-exp, one rounding; a column either side masks with -inf is not guided).  The call
        is ONE padded batch of 2B token rows -- rows [0, B) the prompts, rows [B, 2B) their negative prompts, both padded at
        the right to the longer length under one key mask (attention_mask or ones over negative_prompt_attention_mask or
        ones) -- on the path attention_mask= built: the masked prefill, the compacted cache, token 0 from each row's last
        valid hidden row, the per-sample-position step kernels; two prompts of equal length without padding run the
        unpadded path at 2B rows.  The layers, the cache, the lm_head and the quantised copies see 2B rows; ops.cfg_combine
        then writes the guided scores into rows [0, B), and the processors, the emit, the sampler and the
        log-probabilities see B -- HF's order: guidance first among the processors, the warpers last, the
        log-probabilities those of the guided scores, renormalised.  The emitted token feeds both rows of its sample (two
        gathers into one [2B, D] buffer); on the hipGraph path all of it is inside the captured step: still one replay per
        token.  Composes with decode_weights (their limit becomes 2B <= 32), kv_cache, sampling, the processors,
        log-probabilities, a padded attention_mask, use_cache=False (the 2B prefixes recomputed under the growing mask, any
        dtype) and LoRA.  ValueError naming the condition for a scale that is not a finite number, guidance without a
        negative prompt (HF's fallback to the prompt's last token is not built), both forms of the negative prompt, a
        negative batch, hidden size, dtype or mask shape that does not match, num_beams > 1 and prompt_lookup_num_tokens >
        0 (not built), and for use_cache=True with fp32 parameters or a shape outside ops.decode_attn_ok when the
        assembled batch is padded (use use_cache=False).  None or 1 (default): off -- the negative prompt is ignored,
        nothing is allocated, launched or read.  What guidance does to the quality of a trained checkpoint's answers is
        unmeasured.

        stop_sequences and bad_words_ids, each a list of token-id lists: what TGI's stop_sequences / vLLM's stop / HF's
        stop_strings give at token level, and HF's argument of the same name (NoBadWordsLogitsProcessor).  Both are
        matched on the device against a table built once per call (the rules are written down in include/macaw_hip.h
        and restated in tests/stop_ref.py).  stop_sequences: a sample that has not finished finishes at the step whose
        token makes its GENERATED tokens end with one of the sequences -- the window never reaches into the prompt -- and
        the finished flag then does what eos does: the matched sequence stays in the output, pad_token_id follows, the
        loop ends once every sample has finished, and the returned width is the column at which the last one did, by
        eos or by a sequence, on every path.  One launch (ops.stop_match) directly behind the emit and in front of the
        log-probabilities, so the last token of a stop sequence keeps its real log-probability and the columns behind
        it hold 0.0; min_new_tokens keeps concerning eos alone, as in HF.  bad_words_ids: the last id of a sequence of n
        ids gets -inf when n == 1, and when the history (the processors' history: the prompt's ids where input_ids is
        given, valid ids only under a padded mask, then the generated tokens; a match may straddle the two) ends with
        its first n - 1 ids.  One launch (ops.seq_ban) behind ops.logits_process and in front of every selection,
        which gives HF's chain; a sequence equal to [eos_token_id] is dropped, as in HF.  Two deliberate differences:
        HF skips a sequence while the history is shorter than n and can therefore emit a banned n-gram as a history's
        first n ids, here L >= n - 1 suffices and a banned sequence is never emitted (identical wherever L >= n); HF
        adds -inf, here the column is set to -inf whatever it held.  Log-probabilities score the banned logits, under
        guidance both see the samples' guided rows.  On the hipGraph path both launches are inside the captured step:
        still one replay per token, the host reads nothing more.  Compose with decode_weights, kv_cache, sampling, the
        processors, a padded mask, log-probabilities, guidance, use_cache=False (any dtype) and LoRA.  ValueError naming
        the argument for a value that is not a non-empty list of non-empty lists of integers >= 0, more than 65536
        sequences, a sequence longer than 64, and either argument with num_beams > 1 or prompt_lookup_num_tokens > 0
        (not built).  None (default): nothing is allocated, launched or read.

        num_samples=n in [1, 32] with do_sample=True: parallel sampling, n samples drawn from every prompt (vLLM's and
        OpenAI's n; HF's num_return_sequences under do_sample, which here stays a beam argument).  Returns ids [B * n,
        width], row b * n + j sample j of prompt b, pad_token_id behind each row's own end.  The random number of (row r,
        new token t) is the counter hash of (seed, t, r): what a batch of B * n repeated prompts draws, so the call is that
        batch up to the last bits of its arithmetic (the prefill's GEMMs see B rows, and the repeated batch may select
        another attention form).  The prefill, and with MM_LLMs the towers and the alignment, run ONCE per prompt at B
        rows into a prompt cache [B, S0, 2D] per layer; the rows' own tokens go to a tail cache [B * n, max_new_tokens,
        2D]; the prompt's last hidden row is gathered to its n rows, and every decode step runs B * n token rows whose
        attention (ops.decode_step_attn_shared, engine.SharedPrompt) reads the one copy of the prompt's keys -- the prompt is
        not stored n times, and what its rows re-read comes from cache.  Still one hipGraph replay per token, and the host reads nothing
        new; decode_graph=False, MACAW_NO_DECODE_GRAPH and max_new_tokens <= 2 run the same launches kernel by kernel at a
        device position.  Composes with decode_weights (their limit becomes B * n <= 32), temperature / top_k / top_p,
        the processors and bad_words_ids (the history of row r is its prompt's ids followed by its own tokens),
        stop_sequences (each row ends by itself), log-probabilities, a padded attention_mask (the compacted prompt cache,
        one offset per prompt), LoRA, and use_cache=False (the prompt repeated n times through the recompute loop; any
        dtype; test reference).  ValueError naming the condition for n not an integer in [1, 32]; for n > 1 with
        do_sample=False (n identical greedy rows: HF refuses it too), with num_beams > 1, prompt_lookup_num_tokens > 0,
        guidance_scale or kv_cache="fp8" (not built); and for n > 1 with use_cache=True and fp32 parameters or a shape
        outside ops.shared_attn_ok / ops.decode_attn_ok (use use_cache=False).  1 (default): today's call -- nothing is
        allocated, gathered or launched differently.

        return_session=True and session=s: multi-turn sessions over a kept KV cache (GenerateSession states the rule; it
        is written down in include/macaw_hip.h next to mk_flash_attn_varlen_fwd).  A sample's history is built turn by
        turn: the valid tokens of the turn's prompt, then the turn's generated tokens up to and including the sample's
        final token -- its eos, the last id of the stop sequence that ended it, or its last token at max_new_tokens; pads
        behind it never enter.  A continued call returns for every sample what a fresh call would return for that sample
        alone on history + valid tokens of the new prompt, positions 0 ... len - 1, up to the last bits of its arithmetic
        (other GEMM row counts, another attention form).  The final token of a turn was emitted but never fed: it is the
        session's pending token and becomes row 0 of the next prefill; no extra step is run for it.
        return_session=True: the result becomes (result, session).  A first call runs exactly today's launches and hands
        over its caches instead of dropping them (session_capacity: the cache rows to allocate, at least today's S0 +
        max_new_tokens; more avoids a later regrowth).  Steps that run past a sample's end (a finished sample inside a live
        batch, up to 7 replayed steps) write rows behind its history; they are never read and are overwritten later.
        session=s: input_ids [B, Sn] or inputs_embeds [B, Sn, D], Sn >= 1, optionally attention_mask [B, Sn] with any
        padding pattern (every sample needs a valid token).  The valid rows are left-compacted behind the embedding of the
        pending token (engine.chunk_layout), the caches grow when S0' + max_new_tokens exceeds the capacity (S0' = the
        longest history; ops.copy2d of the valid rows), the new rows run through the layers once -- ops.kv_append_rows into
        the compacted cache, then ops.flash_attn_varlen_fwd over it with the per-sample lengths read on the device (head
        sizes outside that kernel: sample by sample on the host lengths) -- and the existing decode loops follow at one
        device counter plus a per-sample offset, as for a padded batch: still one hipGraph replay per token, and the host
        reads nothing new per token.  s is updated IN PLACE (and returned as well under return_session=True).  Composes with
        decode_weights, sampling, the logits processors and bad_words_ids (their history is s.ids[b] followed by this
        call's valid input_ids; a turn given as embeddings contributes its generated tokens only), stop_sequences (the
        window never reaches in front of this call's generated tokens), log-probabilities and LoRA.  The sampler's counter
        hash uses this call's output column: pass another seed per turn for fresh randomness.  ValueError naming the
        condition, before anything is allocated, for either argument with use_cache=False, num_beams > 1, num_samples > 1,
        prompt_lookup_num_tokens > 0, guidance_scale, kv_cache="fp8" (no quantised attention over several new positions),
        fp32 parameters or a shape outside ops.decode_attn_ok (the continuation needs the per-sample-position step
        kernels); with session= also for a batch, hidden size, dtype, device or layer count that does not match the
        session, Sn < 1, a sample without a valid token and an object that is no GenerateSession.  Defaults (None, False,
        None): not one launch differs.

        adapter_names=[...] (peft's mixed adapter batches, vLLM's per-request LoRA): one name per sample out of the model's
        lora.AdapterBank (model._lora_bank), "__base__" for none, so one batch serves several fine-tuned adapters of the
        base model, or an adapter next to it.  Nothing is merged: the base launches stream the STORED weights -- with
        decode_weights their cached quantised copies, made once -- and the 16-bit adapters go on top.  The prefill adds them
        per run of consecutive samples with the same adapter (the MFMA kernels of csrc/lora.hip on the run's rows); a decode
        step wraps each of its four streamed linears in ops.lora_bgmv_shrink / ops.lora_bgmv_expand_ (csrc/lora_bgmv.hip),
        which read each row's adapter index on the device, so a step still is one hipGraph replay -- of 5 + 8 launches per
        layer.  Those small launches are latency: for ONE adapter the merged path (a live get_peft_model / load_lora adapter
        and no adapter_names) stays the faster one and the default (profiles/decode_adapters_generate.txt).  A row's
        tokens do not depend on the other rows' adapters, bit for bit.  Composes with greedy and sampling, attention_mask,
        decode_weights, kv_cache="fp8", the logits processors, stop sequences, bad words and log-probabilities; the eager
        loop (decode_graph=False) runs the same step launches one by one.  ValueError naming the condition for an unknown
        name, a wrong count of names, a model without a bank or with a live adapter as well, fp32, use_cache=False, unfused
        storage, more than 32 rows, a shape outside ops.decode_attn_ok, num_beams > 1, num_samples > 1,
        prompt_lookup_num_tokens > 0, guidance_scale and sessions (each maps rows to samples in its own way: not built).
        None (the default): not one launch differs.

        grammar=g: grammar-constrained decoding -- what vLLM's guided_regex / guided_choice, TGI's grammar and outlines
        give, and HF's prefix_allowed_tokens_fn without its Python callback per token.  g is a grammar.TokenDFA
        (TokenDFA.from_regex(pattern, vocab), .from_choices(token-id lists), .from_edges(...)), applied to every row, or a
        list with one entry per prompt, each a TokenDFA or None for an unconstrained row; distinct objects go into one
        device table back to back.  The rule is written down in include/macaw_hip.h and restated in
        tests/grammar_ref.py: a row may only emit tokens its current state allows, eos exactly in accepting states, and a
        row whose state becomes terminal (accepting, nothing may follow) finishes there as at a stop sequence -- the
        completing token stays in the output with its real log-probability, pad_token_id follows, and the returned width
        is the column at which the last row finished.  One launch (ops.grammar_mask) sets the other columns to -inf
        behind ops.logits_process and ops.seq_ban and in front of every selection, token 0 included; one launch
        (ops.grammar_advance) moves the per-row state right behind the emit, in front of ops.stop_match.  Table, states
        and ends live on the device: on the hipGraph path both launches are inside the captured step, still one replay
        per token, and the host reads nothing more.  The eager loops (decode_graph=False, MACAW_NO_DECODE_GRAPH,
        max_new_tokens <= 2), the padded-batch loops and use_cache=False (any dtype) run the same two launches.
        Composes with decode_weights, kv_cache="fp8", sampling (mask first, then the warpers: top_k counts allowed
        columns), the processors, bad_words_ids, stop_sequences, log-probabilities (scored on the masked logits, i.e.
        renormalised over the allowed set, as in HF), a padded mask, guidance (on the B guided rows), num_samples (each
        prompt's start state repeats n times), LoRA and adapter_names.  Two limits: max_new_tokens can cut an answer
        short (check with g.walk(ids) / g.is_accepting), and without an eos_token_id an accepting state that still has
        allowed tokens never ends by itself.  Should the other processors ban every column a state allows, the row is
        marked broken and finishes.  ValueError naming the condition for an object that is not a TokenDFA, num_beams > 1,
        prompt_lookup_num_tokens > 0, session= / return_session=True (grammars along beams, through the verify step and
        across sessions are not built), a list of the wrong length and a vocabulary size that is not the model's.  None
        (default): nothing is allocated, launched or read.

        frequency_penalty, presence_penalty, logit_bias: the per-request controls of the OpenAI API, with OpenAI's and
        vLLM's semantics (the rule: include/macaw_hip.h, "Per-request penalties"; restated in tests/penalties_ref.py).
        A token generated cnt > 0 times has frequency_penalty * cnt + presence_penalty SUBTRACTED from its logit --
        additive, proportional to the count, and blind to the prompt, where repetition_penalty is multiplicative,
        idempotent and counts the prompt; logit_bias {token id: bias} is ADDED to its tokens at every step, token 0
        included.  Each penalty is a float, or a sequence / tensor of one float per prompt, finite and in [-2, 2];
        logit_bias is one dict for every prompt or a list with one dict | None per prompt, integer ids in [0, V), finite
        values in [-100, 100], at most 1024 entries per row: a batch may mix requests, every value is per row.  One launch
        (ops.logits_penalize) behind ops.logits_process and in front of ops.seq_ban, the grammar's mask, the
        log-probabilities and every selection, in every loop, the counts read on the device: the graph loop stays one
        hipGraph replay per token.  So bans and the grammar have the last word (a +100 bias cannot lift a banned
        token), log-probabilities are scored on the biased row, and repetition_penalty is applied first (vLLM adds the
        bias in front of it; the two differ only for a token both name).  Composes with sampling and the warpers,
        the processors, stop sequences, bad_words_ids, grammars, log-probabilities, guidance (on the guided row), a
        padded mask, use_cache=False, num_samples (a prompt's values go to each of its rows), decode_weights,
        kv_cache, LoRA and adapter_names, and with sessions, where the count restarts with every call: this call's
        generated tokens only, not those of earlier turns.  ValueError naming the condition for a value out of range, a
        wrong count, a bad id or value, more than 1024 entries, another type, num_beams > 1 and
        prompt_lookup_num_tokens > 0 (penalties along beams and behind the verify step are not built).  With the defaults
        (0.0, 0.0, None) nothing is allocated or launched.

        sampling_params=[...]: per-request sampling, one entry per prompt (OpenAI's temperature / top_p / seed per
        request, vLLM's one SamplingParams per prompt), so a batch mixes greedy and sampled requests, temperatures,
        filters and seeds.  An entry is None or a dict out of temperature, top_k, top_p, min_p, typical_p,
        epsilon_cutoff, eta_cutoff, seed; a missing key takes this function's own default (1.0, 50, 1.0, None, 1.0, 0.0,
        0.0, None) and the values obey the rules of the scalar arguments.  None, or temperature == 0, makes the prompt
        greedy (its other keys are validated all the same); seed=None gives the prompt a fresh 63-bit seed from torch's
        default CPU generator, drawn in prompt order (torch.manual_seed governs them).  The values go into one device
        table (ops.SampleTable; the rule: include/macaw_hip.h, "Per-row sampling table", restated in
        tests/sampling_params_ref.py) that the selection launch reads per row: ops.sample_rows_table in the eager loops,
        ops.decode_emit_sample_table inside the captured step -- still one hipGraph replay per token -- in place of the
        scalar launch, so everything in front of and behind the selection (a padded mask, use_cache=False, guidance on
        its B guided rows, sessions, adapter_names, a grammar, the processors, the penalties, stop sequences,
        log-probabilities, decode_weights, kv_cache) runs as it does for do_sample=True.  A greedy row gets the argmax
        bit for bit.  A sampled row's random number is the counter hash of (its seed, the output column, its stream
        index), the stream index being 0, and j for row b * n + j under num_samples=n: a request's draws depend on its
        own seed, the output column and its sample index, never on its place in the batch, and they are the draws the
        scalar call makes for it at batch 1 -- sampling_params=[d] at B = 1 returns the ids of do_sample=True, **d.  The
        limit: the SELECTION is position-independent; the logits in front of it come from linears that choose their
        kernel by the row count, so their last bits, and with them a draw that falls on a boundary, can differ between
        batch sizes.  A list whose entries are all greedy is the greedy call: no table, no other launch.  ValueError
        naming the condition, before anything is allocated, for the list together with do_sample=True (two ways to say
        it), a value that is not a list or tuple, a wrong length, an entry that is neither None nor a dict, an unknown
        key, a bad value, num_beams > 1, prompt_lookup_num_tokens > 0 and num_samples > 1 with a greedy entry (n
        identical rows).  Out of scope: per-row max_new_tokens, eos, processors (repetition_penalty and its neighbours)
        and stop sequences, per-request sampling along beams or behind the prompt-lookup verify step, and any tuning of
        the selection launch itself.  None (default): not one launch, allocation, host read or message differs."""
        # ---- refusals (a): what the arguments alone decide, before the model is touched
        K = beam_check("generate", num_beams)
        rows_of = inputs_embeds if inputs_embeds is not None else input_ids      # its shape[0]: the prompts
        proc = _processors_check("generate", repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        if proc is not None and K > 1:
            on = [f"{k}={v!r}" for k, v, off in (("repetition_penalty", repetition_penalty, 1.0),
                                                  ("no_repeat_ngram_size", no_repeat_ngram_size, 0),
                                                  ("min_new_tokens", min_new_tokens, 0)) if v != off]
            raise ValueError(f"generate({', '.join(on)}) with num_beams={K}: logits processors along each beam's "
                             "back-tracked history are not built; use num_beams=1")
        if decode_weights not in (None, "fp8", "mxfp4"):
            raise ValueError(f"generate: decode_weights must be None, 'fp8' or 'mxfp4', got {decode_weights!r}")
        if kv_cache not in (None, "fp8"):
            raise ValueError(f"generate: kv_cache must be None or 'fp8', got {kv_cache!r}")
        G = _lookup_check("generate", prompt_lookup_num_tokens, max_matching_ngram_size)
        if G:                     # what prompt lookup does not compose with
            why = None
            if K > 1:
                why = f"num_beams={K} > 1 (lookup along beams is not built)"
            elif do_sample:
                why = "do_sample=True (sampling-based acceptance is not built)"
            elif proc is not None:
                why = ("a logits processor (repetition_penalty, no_repeat_ngram_size or min_new_tokens: lookup behind "
                       "processors is not built)")
            elif kv_cache == "fp8":
                why = "kv_cache='fp8' (there is no multi-row step over the e4m3 cache: not built)"
            elif not use_cache:
                why = "use_cache=False (the verify step runs on the KV cache: not built without it)"
            elif attention_mask is not None and not bool((attention_mask != 0).all()):
                why = "a padded attention_mask (lookup over a ragged cache is not built)"
            elif rows_of.shape[0] * (G + 1) > 32:
                why = (f"B x (G + 1) = {rows_of.shape[0]} x {G + 1} = {rows_of.shape[0] * (G + 1)} rows: a verify step takes "
                       "at most 32 (B * Q <= 32; a wider step is not built)")
            elif inputs_embeds is not None and inputs_embeds.dtype not in _16BIT:
                why = (f"fp32 parameters ({inputs_embeds.dtype}): the multi-row step attention takes bf16 / fp16 (not built "
                       "for fp32)")
            if why is not None:
                raise ValueError(f"generate(prompt_lookup_num_tokens={G}): {why}")
        pen = None                # frequency_penalty / presence_penalty / logit_bias (None: off, nothing below runs)
        if not (type(frequency_penalty) in (int, float) and frequency_penalty == 0 and type(presence_penalty) in (int, float)
                and presence_penalty == 0 and logit_bias is None):                           # not the defaults
            pen = _penalties_check("generate", frequency_penalty, presence_penalty, logit_bias, rows_of.shape[0])
        if pen is not None:
            what = "generate(frequency_penalty=, presence_penalty=, logit_bias=)"
            if K > 1:
                raise ValueError(f"{what} with num_beams={K}: penalties along each beam's back-tracked history are not "
                                 "built; use num_beams=1")
            if G:
                raise ValueError(f"{what} with prompt_lookup_num_tokens={G}: lookup behind "
                                 "penalties is not built")
        n_top = None              # return_logprobs: the top columns per token (None: off, nothing below runs)
        if not (return_logprobs is False and type(top_logprobs) is int and top_logprobs == 0):   # not the defaults
            n_top = _logprobs_check("generate", return_logprobs, top_logprobs, K, G)
        cfg = None                # guidance_scale: the scale (None: off, the negative prompt is ignored, nothing below runs)
        if guidance_scale is not None:
            cfg = _guidance_check("generate", guidance_scale)
        if cfg is not None:
            what = f"generate(guidance_scale={guidance_scale!r})"
            if negative_prompt_ids is None and negative_inputs_embeds is None:
                raise ValueError(f"{what} without a negative prompt: pass negative_prompt_ids or negative_inputs_embeds (HF's "
                                 "fallback to the prompt's last token is not built)")
            if negative_prompt_ids is not None and negative_inputs_embeds is not None:
                raise ValueError(f"{what}: both negative_prompt_ids and negative_inputs_embeds were given; pass one")
            if K > 1:
                raise ValueError(f"{what} with num_beams={K}: guidance along beams is not built; use num_beams=1")
            if G:
                raise ValueError(f"{what} with prompt_lookup_num_tokens={G}: a guided verify step is not built")
        stop = bad = None         # stop_sequences / bad_words_ids as lists (None: off, nothing below runs)
        if stop_sequences is not None or bad_words_ids is not None:
            stop, bad = _stopping_check("generate", stop_sequences, bad_words_ids, eos_token_id, K, G)
        sample = None
        if do_sample:
            temperature, top_k, top_p = _sampling_check("generate", temperature, top_k, top_p)
            if seed is None:
                seed = int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64))
            sample = (temperature, top_k, top_p, int(seed)) + _warpers_check("generate", min_p, typical_p, epsilon_cutoff,
                                                                             eta_cutoff)
        sp = None                 # sampling_params: per prompt None (greedy) or its values (None: off, nothing below runs)
        if sampling_params is not None:
            what = "generate(sampling_params=)"
            if do_sample:
                raise ValueError(f"{what} with do_sample=True: two ways to say how tokens are selected; pass the scalar "
                                 "arguments or the list, not both")
            sp = _sampling_params_check("generate", sampling_params, rows_of.shape[0])
            if K > 1:
                raise ValueError(f"{what} with num_beams={K}: per-request sampling along beams is not built; use "
                                 "num_beams=1")
            if G:
                raise ValueError(f"{what} with prompt_lookup_num_tokens={G}: per-request sampling behind the verify step "
                                 "is not built")
        N = 1                     # num_samples: the rows per prompt (1: off, nothing below runs)
        if not (type(num_samples) is int and num_samples == 1):
            N = _num_samples_check("generate", num_samples)
        if N > 1 and sp is not None and any(r is None for r in sp):
            raise ValueError(f"generate(num_samples={N}) with a greedy entry in sampling_params (entry "
                             f"{[r is None for r in sp].index(True)}): greedy decoding would return {N} identical rows for "
                             "that prompt; give every entry a temperature > 0")
        if sp is not None and all(r is None for r in sp):
            sp = None             # every prompt greedy: today's greedy call, no table and no other launch
        if N > 1:
            what = f"generate(num_samples={N})"
            if not do_sample and sp is None:
                raise ValueError(f"{what} with do_sample=False: greedy decoding would return {N} identical rows per prompt; "
                                 "pass do_sample=True")
            if K > 1:
                raise ValueError(f"{what} with num_beams={K}: parallel samples of a beam search are not built; use "
                                 "num_beams=1")
            if G:
                raise ValueError(f"{what} with prompt_lookup_num_tokens={G}: a verify step over a shared prompt cache is not "
                                 "built")
            if cfg is not None:
                raise ValueError(f"{what} with guidance_scale={guidance_scale!r}: guided parallel samples are not built")
            if kv_cache == "fp8":
                raise ValueError(f"{what} with kv_cache='fp8': a quantised shared-prompt cache is not built")
        sess = session is not None or bool(return_session)      # sessions (False: nothing below runs for them)
        if sess:
            why = _session_refusal(session, return_session, use_cache, K, N, G, cfg, kv_cache)
            if why is not None:
                raise ValueError(why)
            if session_capacity is not None and (isinstance(session_capacity, bool) or
                                                 not isinstance(session_capacity, numbers.Integral) or session_capacity < 1):
                raise ValueError(f"generate: session_capacity must be None or an integer >= 1, got {session_capacity!r}")
        bank = None               # adapter_names: the model's AdapterBank (None: off, nothing below runs)
        if adapter_names is not None:
            what = "generate(adapter_names=)"
            bank = getattr(self, "_lora_bank", None)
            why = None
            if bank is None:
                why = "the model has no adapter bank (lora.AdapterBank(model).add(name, directory))"
            elif getattr(self, "_lora", None) is not None:
                why = ("the model also carries a live adapter (get_peft_model / load_lora), which generate() merges; "
                       "merge_and_unload() it or put it into the bank")
            elif K > 1:
                why = f"num_beams={K} > 1 (adapters along beams are not built)"
            elif N > 1:
                why = f"num_samples={N} > 1 (adapters over a shared prompt cache are not built)"
            elif G:
                why = f"prompt_lookup_num_tokens={G} (an adapted verify step is not built)"
            elif cfg is not None:
                why = f"guidance_scale={guidance_scale!r} (adapters on the guided pair of rows are not built)"
            elif sess:
                why = "session= / return_session=True (a session does not keep its rows' adapters: not built)"
            elif not use_cache:
                why = "use_cache=False (the recompute loop runs the training layer, which has no per-row adapters)"
            if why is not None:
                raise ValueError(f"{what}: {why}")
        gram = None               # grammar=: one TokenDFA | None per prompt (None: off, nothing below runs)
        if grammar is not None:
            gram = _grammar_check("generate", grammar, K, G, sess)
        no_graph = _no_decode_graph(decode_graph, max_new_tokens)
        graph = no_graph is None  # the decode step is captured in a hipGraph (the greedy loop also needs decode_attn_ok)

        emb_w = self.model.embed_tokens.weight
        if inputs_embeds is None:
            inputs_embeds = ops.embedding_fwd(emb_w, input_ids.long().reshape(-1)).view(*input_ids.shape, -1)
        _dev_check(inputs_embeds)
        n_prompts, rows_per = inputs_embeds.shape[0], N      # (grammar=: the prompts and the rows each of them decodes)
        if N > 1 and not use_cache:   # the prompt repeated N times through the recompute loop: a batch of B * N rows
            inputs_embeds = inputs_embeds.repeat_interleave(N, 0)
            attention_mask = attention_mask.repeat_interleave(N, 0) if attention_mask is not None else None
            input_ids = input_ids.repeat_interleave(N, 0) if input_ids is not None else None
            N = 1
        B, S0, D = inputs_embeds.shape
        dev, dtype = inputs_embeds.device, inputs_embeds.dtype
        chunk = None              # session=: the continued prefill's layout (None: a first call, nothing below runs)
        prompt_ids = None         # sessions: per sample the valid ids of this call's prompt (None: embeddings)
        if session is not None:
            what, Sn = "generate(session=)", S0
            mine = dict(batch=B, hidden=D, dtype=dtype, device=dev, layers=len(self.model.layers))
            theirs = dict(batch=session.batch, hidden=session._hidden, dtype=session._dtype, device=session._device,
                          layers=len(session._kvc))
            for k in mine:
                if mine[k] != theirs[k]:
                    raise ValueError(f"{what}: {k} {mine[k]} of this call does not match the session's ({theirs[k]})")
            if Sn < 1:
                raise ValueError(f"{what}: the new prompt needs at least one token (Sn >= 1), got {Sn}")
            valid = torch.ones((B, Sn), dtype=torch.bool)
            if attention_mask is not None:
                if tuple(attention_mask.shape) != (B, Sn):
                    raise ValueError(f"{what}: attention_mask should be of size {(B, Sn)}, but is {tuple(attention_mask.shape)}")
                valid = attention_mask.cpu() != 0
            try:
                chunk, ck_pos, ck_last, S0, ck_off = eng.chunk_layout(session._cached_host, valid.sum(1).tolist(), dev)
            except ValueError as e:
                raise ValueError(f"{what}: attention_mask: {e}") from None
            Sq = chunk.slot.shape[1]
            # row (b, j) of the prefill out of [pending's embeddings (B rows); the prompt's (B * Sn rows)]: the pending token,
            # the valid rows in order, then the last of them again as filler
            src = [torch.cat([torch.tensor([b]), torch.nonzero(valid[b]).flatten() + B + b * Sn]) for b in range(B)]
            ck_src = torch.stack([torch.cat([r, r[-1:].expand(Sq - r.numel())]) for r in src]).reshape(-1).to(dev)
            if input_ids is not None and tuple(input_ids.shape) == (B, Sn):
                prompt_ids = [input_ids[b].cpu()[valid[b]].tolist() for b in range(B)]
            attention_mask = None     # (consumed: from here on S0 = S0', the longest history, where the step counter starts)
        elif return_session and input_ids is not None:
            if attention_mask is not None and tuple(input_ids.shape) == tuple(attention_mask.shape):
                prompt_ids = [input_ids[b].cpu()[attention_mask[b].cpu() != 0].tolist() for b in range(B)]
            else:
                prompt_ids = input_ids.cpu().tolist()
        Bs, Sc, own_mask = B, S0, attention_mask     # the samples, their prompt's length and mask as the caller gave them
        if cfg is not None:       # ONE batch of B = 2 Bs token rows under one key mask: the padded-batch path from here on
            neg = negative_inputs_embeds
            if neg is None:
                if negative_prompt_ids.dim() != 2 or negative_prompt_ids.shape[0] != Bs:
                    raise ValueError(f"generate(guidance_scale={guidance_scale!r}): negative_prompt_ids should be [{Bs}, Sn], "
                                     f"but is {tuple(negative_prompt_ids.shape)}")
                neg = ops.embedding_fwd(emb_w, negative_prompt_ids.to(dev).long().reshape(-1)).view(
                    *negative_prompt_ids.shape, -1)
            inputs_embeds, attention_mask = _guided_batch(guidance_scale, inputs_embeds, attention_mask, neg,
                                                          negative_prompt_attention_mask)
            B, S0 = inputs_embeds.shape[:2]
        pad = pad_token_id if pad_token_id is not None else (eos_token_id or 0)
        eps = self.model.norm.variance_epsilon
        layers = self.model.layers
        V = self.lm_head.weight.shape[0]
        hd = D // layers[0].self_attn.num_heads
        if pen is not None:       # logit_bias: the ids against the vocabulary, now that it is known
            _penalties_check("generate", frequency_penalty, presence_penalty, logit_bias, n_prompts, V)
        Tmax = S0 + max_new_tokens + G        # rows of the KV cache (prompt lookup: the G draft rows behind the last token)
        if sess:                  # a session's caches: the capacity asked for, or the one it has while that suffices
            need = Tmax
            if session_capacity is not None and session_capacity < need and session is None:
                raise ValueError(f"generate(return_session=True): session_capacity={session_capacity} is below the {need} "
                                 f"rows this call needs (S0 + max_new_tokens = {S0} + {max_new_tokens})")
            Tmax = max(need, session_capacity or 0)
            if session is not None and need <= session.capacity:
                Tmax = session.capacity

        # ---- refusals (b): what needs the shapes, the dtype, the head size or the mask, before anything is allocated
        # a padded batch: engine.Ragged, the prefill's positions, the flat index of each sample's last valid row
        ragged = rg_pos = rg_last = None
        if attention_mask is not None:
            padded = eng.ragged_from_mask(attention_mask.to(dev), B, S0)        # None for a mask without a zero
            if padded is not None:
                ragged, rg_pos, rg_last = padded
        hist = hist_len = None    # the prompt's ids as history (the processors' or the lookup's): [B, P] int64, count per row
        if (proc is not None or bad is not None) and session is not None:
            # the session's known ids, then this call's valid input_ids
            rows = [r + (prompt_ids[b] if prompt_ids is not None else []) for b, r in enumerate(session._ids)]
            hist = torch.zeros((B, max(1, max(len(r) for r in rows))), dtype=torch.long)
            for b, r in enumerate(rows):
                hist[b, :len(r)] = torch.tensor(r, dtype=torch.long)
            hist, hist_len = hist.to(dev), torch.tensor([len(r) for r in rows], dtype=torch.int32, device=dev)
        elif (proc is not None or bad is not None) and input_ids is not None:
            hist_rg = ragged      # the padding the history leaves out: with guidance the caller's own, of the samples' rows
            if cfg is not None and ragged is not None:
                own = own_mask is not None and not bool((own_mask != 0).all())
                hist_rg = eng.Ragged(ragged.kmask[:Bs, :Sc], ragged.slot[:Bs, :Sc], ragged.t_off[:Bs]) if own else None
            hist, hist_len = _prompt_history(input_ids, Bs, dev, "the processors' prompt history", hist_rg)
        no_attn = _attn_refusal(dtype, hd, Tmax)      # why the per-sample-position step kernels do not take this call
        if K > 1:
            beam_check("generate", K, num_return_sequences, V, do_sample, kv_cache, ragged is not None, length_penalty)
            why = _attn_refusal(dtype, hd, S0 + max_new_tokens) if use_cache else None
            if why is not None:
                raise ValueError(f"generate(num_beams={K}) with use_cache=True: {why}; the beam step attention takes bf16 / "
                                 "fp16 inside ops.decode_attn_ok: pass use_cache=False")
        if N > 1:                 # (use_cache=True: the other case became a batch of B * N rows above)
            why = no_attn
            if why is None and not ops.shared_attn_ok(dtype, hd, N):
                why = f"ops.shared_attn_ok is false for head size {hd} and {N} rows per prompt"
            if why is not None:
                raise ValueError(f"generate(num_samples={N}) with use_cache=True: {why}; the shared-prompt step attention "
                                 "takes bf16 / fp16 inside ops.shared_attn_ok and ops.decode_attn_ok: pass use_cache=False")
        if decode_weights is not None:
            _decode_fp8_check(dtype, hd, B * N, S0, max_new_tokens, use_cache, no_graph, value=decode_weights, beams=K,
                              guided=cfg is not None)
        if kv_cache == "fp8":
            _decode_fp8_check(dtype, hd, B, S0, max_new_tokens, use_cache, no_graph, switch="kv_cache")
        if G:
            why = _attn_refusal(dtype, hd, Tmax, G + 1)
            if why is not None:
                raise ValueError(f"generate(prompt_lookup_num_tokens={G}): {why}: the multi-row step attention is not built "
                                 "for it")
            if input_ids is not None:
                hist, hist_len = _prompt_history(input_ids, B, dev, "the lookup history")
        if sess and no_attn is not None:
            raise ValueError(f"generate({'session=' if session is not None else 'return_session=True'}): {no_attn}; a "
                             "continued call needs the per-sample-position decode kernels, which take bf16 / fp16 inside "
                             "ops.decode_attn_ok")
        ad_idx = None             # adapter_names: per sample its adapter's index in the bank, -1 for "__base__"
        if bank is not None:
            what = "generate(adapter_names=)"
            names = list(adapter_names)
            if len(names) != B:
                raise ValueError(f"{what}: {len(names)} names for {B} samples (one per sample, '__base__' for none)")
            ad_idx = bank.indices(names)          # (ValueError for an unknown name)
            why = no_attn
            if dtype not in _16BIT:
                why = f"fp32 parameters ({dtype}): the adapter kernels of a decode step take bf16 / fp16"
            elif any(w is None for lyr in layers for w in lyr.fused_weights()):
                why = ("unfused q/k/v or gate/up storage (the adapted decode step is the five-launch one on the fused "
                       "q|k|v and gate|up weights: fuse_projections())")
            elif B > 32:
                why = f"{B} rows: an adapted decode step takes at most 32"
            if why is not None:
                raise ValueError(f"{what}: {why}")
        if ragged is not None and use_cache and no_attn is not None:
            call = ("generate(attention_mask=) with a padded mask" if cfg is None else
                    f"generate(guidance_scale={guidance_scale!r}) with prompts of two lengths or a padded mask")
            raise ValueError(f"{call} and use_cache=True: {no_attn}; the per-sample-position decode kernels take bf16 / "
                             "fp16 inside ops.decode_attn_ok and there is no masked attention over a cache: pass "
                             "use_cache=False")
        if gram is not None:
            gram = _grammar_rows(gram, n_prompts, V)
            if all(g is None for g in gram):          # a list of unconstrained rows: the plain call
                gram = None

        if N > 1:                 # from here on the emits, the books and the processors count the B * N rows
            Bs = B * N
            if hist is not None:  # row r's history starts with its prompt's ids
                hist, hist_len = hist.repeat_interleave(N, 0).contiguous(), hist_len.repeat_interleave(N).contiguous()
        w8_head = None            # decode_weights="fp8" / "mxfp4": (q, scales) of the lm_head, e4m3 in both modes

        def logits(h_last):       # h_last [B, D] -> [B, V] (final norm folded into the lm_head stream)
            if h_last.is_contiguous():
                return eng._stream_linear(h_last, self.lm_head.weight, w8_head, 1, self.model.norm.weight, eps, None, 0)
            _, y, _ = ops.rmsnorm_fwd(h_last, self.model.norm.weight, eps)
            return ops.linear_fwd(y, self.lm_head.weight)

        # the greedy and sampled loops' way from a step's hidden rows to its tokens (beams and lookup have emits of their own)
        chain = None if K > 1 or G else _Selection(
            logits, emb_w, Bs, V, max_new_tokens, eos_token_id, pad, dev, per_prompt=rows_per, sample=sample, params=sp,
            n_top=n_top, proc=proc, hist=hist, hist_len=hist_len, pen=pen, bad=bad, stop=stop, gram=gram, cfg=cfg)

        def beam_out(bs, state):      # the books after the loop -> what generate returns
            n_cols = int(state[1])
            ids, sc = beam_result(bs.hist.cpu(), bs.scores.cpu(), bs.pool_score.cpu(), bs.pool_info.cpu(), bs.done.cpu(),
                                  n_cols, length_penalty, num_return_sequences, pad,
                                  -1 if eos_token_id is None else eos_token_id)
            return (ids.to(dev), sc.to(dev)) if return_beam_scores else ids.to(dev)

        if not use_cache and K > 1:   # the B * K prefixes recomputed per step, the same ops.beam_emit
            state = _step_state(S0, dev)
            bs = ops.BeamState(B, K, max_new_tokens, pad, dev)
            emb = inputs_embeds.contiguous()
            own = torch.arange(B, device=dev).repeat_interleave(K)      # the sample of row (b, j) ...
            base = own * K                                              # ... and the row of its beam 0
            for t in range(max_new_tokens):
                ops.beam_emit(logits(self._hidden_last(emb)), V, 1 if t == 0 else K, pad, eos_token_id, length_penalty,
                              early_stopping, bs, state)
                if t + 1 == max_new_tokens or bool(bs.done.all()):
                    break
                # row (b, j) continues the prefix of its parent (b, parent[j]) with its new token
                emb = _append_column(emb, emb_w, bs.tok, base + bs.hist[t, :, :, 1].reshape(-1).long() if t > 0 else own)
            return beam_out(bs, state)

        if not use_cache:
            emb = inputs_embeds.contiguous()
            mask = ragged.kmask if ragged is not None else None        # grows by a one per new token
            for t in range(max_new_tokens):
                # under a mask token 0 is predicted by each sample's last valid row
                nxt = chain.eager_step(self._hidden_last(emb, mask, rg_last if mask is not None and t == 0 else None), t)
                if chain.finished():
                    break
                # (guidance: the token continues both prefixes of its sample)
                emb = _append_column(emb, emb_w, nxt.contiguous() if cfg is None else torch.cat([nxt, nxt]))
                if mask is not None:
                    mask = torch.cat([mask, torch.ones((B, 1), dtype=mask.dtype, device=dev)], dim=1)
            return chain.eager_result()

        rot = layers[0].self_attn.rotary_emb
        cos, sin = rot.tables(Tmax, dtype, dev)
        kvs = None                # kv_cache="fp8": per layer the f32 scales of the e4m3 cache (kvc: its bytes)
        if kv_cache == "fp8":
            kvc, kvs = zip(*(ops.kv8_cache(B, Tmax, D // hd, hd, dev) for _ in layers))
        elif K > 1:               # one slot per beam; the prompt lives in slot 0 of its sample only
            kvc = [torch.empty((B, K, Tmax, 2 * D), dtype=dtype, device=dev) for _ in layers]
        elif N > 1:               # the prompt's rows once per prompt, the rows' own tokens per row (engine.SharedPrompt)
            kvc = [torch.empty((B, S0, 2 * D), dtype=dtype, device=dev) for _ in layers]
            tails = [torch.empty((B * N, max_new_tokens, 2 * D), dtype=dtype, device=dev) for _ in layers]
        elif session is not None and Tmax == session.capacity:
            kvc = session._kvc
        else:
            kvc = [torch.empty((B, Tmax, 2 * D), dtype=dtype, device=dev) for _ in layers]   # [keys | values]
            if session is not None:   # regrowth: the rows the histories hold move over, the session keeps the new caches
                for old, new in zip(session._kvc, kvc):
                    ops.copy2d(old, new, max(session._cached_host), 2 * D, 2 * D, 2 * D, batch=B,
                               s_src=session.capacity * 2 * D, s_dst=Tmax * 2 * D)
                session._kvc = kvc

        if getattr(self, "_lora", None) is not None:
            # LoRA adapters: the decode path runs on MERGED copies of the adapted weights (W + s B A, csrc/lora.hip),
            # made once for this call and dropped at its end -- temporarily one extra copy of every adapted
            # projection (all seven of a 7B layer: 0.4 GB bf16 per layer, 12.9 GB for 32 layers)
            from .lora import lora_layers, merged_layer_weights
            merged = dict(merged_layer_weights(self, lyr) for _, lyr in lora_layers(self))
        else:
            merged = {}

        stored = []               # per layer its own parameters, as the engine's named weight set
        for lyr in layers:
            a, m = lyr.self_attn, lyr.mlp
            stored.append(eng.LayerWeights(a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, m.gate_proj.weight,
                                           m.up_proj.weight, m.down_proj.weight, *lyr.fused_weights()))

        w8 = None                 # decode_weights="fp8" / "mxfp4": per layer the copies of q|k|v, o, gate|up, down
        if decode_weights is not None:
            probe = torch.empty((B * N * K * (G + 1), 0), dtype=dtype, device=dev)     # the token rows of a step

            def q8(W, own):       # own: a stored parameter (version-keyed cache); else a merged copy of this call
                if W is None or not ops.decode_linear_fp8_ok(probe, W):
                    return None   # outside the plain fp8 domain: this projection keeps its 16-bit launch
                return ops.fp8_weight(W) if own is not None and own.data_ptr() == W.data_ptr() else ops.quantize_fp8_rows(W)

            def q4(W, own):       # the same rule for the MXFP4 copies (K % 128 == 0)
                if W is None or not ops.decode_linear_mxfp4_ok(probe, W):
                    return None
                return ops.mxfp4_weight(W) if own is not None and own.data_ptr() == W.data_ptr() else ops.quantize_mxfp4_rows(W)

            ql = q4 if decode_weights == "mxfp4" else q8     # the layers' projections; the lm_head is e4m3 in both modes

            w8 = []
            for lyr, own in zip(layers, stored):
                if own.wqkv is None or own.wgu is None:
                    raise ValueError(f"generate(decode_weights='{decode_weights}'): unfused q/k/v or gate/up storage (the "
                                     f"{decode_weights} decode step streams the fused q|k|v and gate|up weights: "
                                     "fuse_projections())")
                ws = merged.get(lyr, own)
                w8.append((ql(ws.wqkv, own.wqkv), ql(ws.wo, own.wo), ql(ws.wgu, own.wgu), ql(ws.wd, own.wd)))
            w8_head = q8(self.lm_head.weight, self.lm_head.weight)

        adapt = None              # adapter_names: adapt(layer, copies) -> what travels in llama_layer_cached's w8
        if ad_idx is not None:
            ad_dev = torch.tensor(ad_idx, dtype=torch.int32, device=dev)
            ad_runs, ad_s, ad_groups = bank.runs(ad_idx), bank.scalings(), bank.stacks()

            def adapt(i, copies):
                return eng.Adapters(ad_dev, ad_runs, ad_s, *ad_groups[i], copies)

        def run(x2, Sn, t0, pos=None, t_dev=None, beam=None, spec=None, chunk=None):
            if pos is None:
                pos = (torch.arange(t0, t0 + Sn, dtype=torch.int32, device=dev)).repeat(B)
            for i, lyr in enumerate(layers):
                ws = merged.get(lyr, stored[i])
                w8_i = w8[i] if w8 is not None and t_dev is not None else None
                if adapt is not None:
                    w8_i = adapt(i, w8_i)
                if K > 1 and beam is None:        # the prefill of a beam cache: B rows into slot 0 of every sample
                    cache_i, tmax_i = kvc[i].view(B, K * Tmax, 2 * D), K * Tmax
                elif N > 1:                       # parallel samples: the prefill writes the prompt cache, a step reads both
                    cache_i, tmax_i = (kvc[i], S0) if t_dev is None else (eng.SharedPrompt(kvc[i], tails[i], N, S0), Tmax)
                else:
                    cache_i, tmax_i = kvc[i], Tmax
                x2 = eng.llama_layer_cached(
                    x2, B, Sn, t0, cache_i, tmax_i, pos, cos, sin, lyr.self_attn.num_heads,
                    lyr.input_layernorm.variance_epsilon, ws.wq, ws.wk, ws.wv, ws.wo, ws.wg, ws.wu, ws.wd,
                    lyr.input_layernorm.weight, lyr.post_attention_layernorm.weight, ws.wqkv, ws.wgu, t_dev=t_dev,
                    w8=w8_i,
                    kv8=kvs[i] if kvs is not None else None, ragged=ragged if chunk is None else chunk, beam=beam,
                    spec=spec)
            return x2

        def hand_over(res):       # sessions: the books behind the loop -> what generate returns
            rows = (res.ids if n_top is not None else res).cpu().tolist()
            if chunk is not None:
                start = chunk.k_host
            else:
                start = ragged.kmask.sum(1).cpu().tolist() if ragged is not None else [S0] * B
            books = GenerateSession.book(start, prompt_ids, rows, eos_token_id, stop)
            if session is not None:
                session._advance(*books)
            s = session if session is not None else GenerateSession(kvc, books[0], torch.tensor(books[1]), books[2], D, dev)
            return (res, s) if return_session else res

        if chunk is not None:     # a continued call: the pending token and the new prompt over the kept cache ...
            table = torch.cat([ops.embedding_fwd(emb_w, session._pending), inputs_embeds.reshape(B * Sn, D)])
            h = run(ops.embedding_fwd(table, ck_src), Sq, 0, pos=ck_pos, chunk=chunk)
            last = ops.embedding_fwd(h, ck_last)
            ragged = eng.Ragged(None, None, ck_off)       # ... then the padded batch's steps at S0' + t + t_off[b]
        elif ragged is not None:  # prefill over the padded rows; token 0 comes from each sample's last valid row
            h = run(eng._c2(inputs_embeds, B * S0, D), S0, 0, pos=rg_pos)
            last = ops.embedding_fwd(h.view(B * S0, D), rg_last)
        else:
            h = run(eng._c2(inputs_embeds, B * S0, D), S0, 0)             # prefill
            last = torch.empty((B, D), dtype=dtype, device=dev)
            ops.copy2d(h, last, 1, D, D, D, batch=B, s_src=S0 * D, s_dst=D, src_off=(S0 - 1) * D)
        if N > 1:                 # the prompt's last hidden row, once per row of its samples
            last = ops.embedding_fwd(last, torch.arange(B, device=dev).repeat_interleave(N))
        if G:
            ids, steps = self._generate_lookup(run, logits, last, emb_w, B, G, S0, max_new_tokens, eos_token_id, pad, dev,
                                               max_matching_ngram_size, hist, hist_len, graph)
            return (ids, steps) if return_lookup_stats else ids
        if K > 1:
            return beam_out(*self._generate_beam(run, logits, last, emb_w, B, K, S0, max_new_tokens, eos_token_id, pad, dev,
                                                 length_penalty, early_stopping, graph))
        if graph and ops.decode_attn_ok(dtype, hd, Tmax):
            res = self._generate_graph(run, chain, last, S0, max_new_tokens)
            return hand_over(res) if sess else res
        # the host-position loop (fp32, a shape outside ops.decode_attn_ok), and every eager loop of a padded batch or of
        # parallel samples
        # (parallel samples and adapters take the padded batch's route: a device position)
        dyn = ragged is not None or N > 1 or adapt is not None
        t_dev = torch.tensor([S0], dtype=torch.int32, device=dev) if dyn else None
        for t in range(max_new_tokens):
            nxt = chain.eager_step(last, t)
            if t + 1 == max_new_tokens or chain.finished():
                break
            x = chain.feed(nxt.contiguous())                               # [B, D]
            if dyn:                                                        # the graph path's step launches, one by one
                last = run(x, 1, 0, pos=t_dev, t_dev=t_dev)
                t_dev += 1
            else:
                last = run(x, 1, S0 + t)                                   # decode step
        res = chain.eager_result()
        return hand_over(res) if sess else res

    @torch.no_grad()
    def score(self, inputs_embeds=None, input_ids=None, continuations=None, continuation_ids=None,
              continuation_lengths=None, attention_mask=None, top_logprobs=0, use_cache=True):
        """The log-likelihood of GIVEN answers over a shared prompt (lm-eval's loglikelihood, OpenAI / vLLM echo +
        logprobs over the answer): what multiple-choice evaluation, re-ranking and perplexity of a reference need.

        The rule (include/macaw_hip.h, "Scoring"; tests/score_ref.py).  B prompts; prompt b has L_b valid tokens and
        n_b <= n options; option (b, j) is a token list c[0 ... len - 1], len >= 1, and for g = 0 ... len - 1
            lp[b, j, g] = log_softmax(logits at position L_b + g - 1, given prompt b followed by c[0 ... g - 1])[c[g]]
        -- what a fresh call on the concatenation alone computes, and what generate(return_logprobs=True) reports for a
        token it emitted itself.  A value's arithmetic is ops.token_logprobs' (fp64 log-sum-exp, one rounding).

        The prompt (inputs_embeds [B, S0, D] or input_ids [B, S0]) and attention_mask mean what they mean to generate():
        any padding pattern, L_b the valid tokens of sample b.  The options come as
          continuations         a list of B lists of token-id lists: prompts may have different option counts (absent
                                options are padded to n = the largest), options different lengths; or
          continuation_ids      int64 [B, n, Lc] with continuation_lengths [B, n] (0 = absent), on the device: no value
                                of either is read on the host (lengths are clamped into [0, Lc]; a fed id is clamped
                                into [0, V), a scored id outside it gives NaN) -- the form in which the output of
                                generate(num_samples=n) is re-ranked.
        Returns ScoreResult(token_logprobs f32 [B, n, Lc] (0.0 behind each option's end), lengths int64 [B, n], sums f32
        [B, n] (the fp64 sum in column order, one rounding; -inf for an absent option), top_ids, top_logprobs): with
        top_logprobs = m in [1, 20] the m most likely ids of every scored position, int64 [B, n, Lc, m] (-1 behind the
        end), and their values f32 (0.0 behind the end); otherwise both None.

        use_cache=True.  (1) The prefill runs ONCE per prompt at B rows into a [B, S0, 2D] prompt cache per layer -- the
        launches of generate(num_samples=)'s prefill, a padded batch's compacted cache included.  (2) The prompt's last
        valid hidden row gives, through the final norm and the lm_head at B rows, token 0 of every option.  (3) Token
        g >= 1 is predicted by the hidden row of FED token g - 1: the B * n * F fed rows, F = Lc - 1, go through the
        layers as one GEMM pass (engine.llama_layer_score: ops.linear_fwd, and ops.score_attn over the prompt cache and
        a tail cache per option, at a position per row, dead rows masked on the device); with F = 0 no pass runs.  (4)
        Final norm and lm_head over the fed rows in chunks of SCORE_LOGITS_ELEMS // V rows.  (5) ops.token_logprobs.
        use_cache=False: the reference path and the fallback, every dtype: the B * n concatenations [prompt | option]
        as one padded batch through the ordinary forward under the mask, the prompt recomputed per option.

        A live LoRA adapter (get_peft_model / load_lora) runs on the per-call merged copies, as in generate().  Not
        built: prompt log-probabilities, an e4m3 cache or quantised weights, adapter_names, sessions.

        ValueError, naming the condition, before anything is allocated: both or neither of inputs_embeds / input_ids;
        both or neither continuation form; a batch size other than B; a prompt without options or an empty option (list
        form); a token id outside [0, V) (list form); n > 32; top_logprobs outside [0, 20]; L_b + len beyond the rotary
        table (max_position_embeddings; the tensor form counts Lc for len); an attention_mask of another shape or a
        sample without a valid token; and with use_cache=True fp32 parameters or a shape outside ops.score_attn_ok
        ("use use_cache=False")."""
        if (inputs_embeds is None) == (input_ids is None):
            raise ValueError("score: pass exactly one of inputs_embeds and input_ids")
        src = inputs_embeds if inputs_embeds is not None else input_ids
        if src.dim() != (3 if inputs_embeds is not None else 2) or src.shape[1] < 1:
            raise ValueError(f"score: the prompt should be inputs_embeds [B, S0, D] or input_ids [B, S0] with S0 >= 1, but is "
                             f"{tuple(src.shape)}")
        B, S0 = src.shape[:2]
        dev = src.device
        if isinstance(top_logprobs, bool) or not isinstance(top_logprobs, numbers.Integral) or \
                not 0 <= top_logprobs <= ops.MAX_TOP_LOGPROBS:
            raise ValueError(f"score: top_logprobs must be an integer in [0, {ops.MAX_TOP_LOGPROBS}], got {top_logprobs!r}")
        m = int(top_logprobs)
        emb_w = self.model.embed_tokens.weight
        V, D = self.lm_head.weight.shape[0], emb_w.shape[1]
        lay = eng.score_layout(continuations, continuation_ids, continuation_lengths, B=B, V=V)
        n, F, Lc = lay.n, lay.F, lay.Lc
        ragged = rg_pos = rg_last = None
        n_valid = [S0] * B
        if attention_mask is not None:
            padded = eng.ragged_from_mask(attention_mask.to(dev), B, S0)        # None for a mask without a zero
            if padded is not None:
                ragged, rg_pos, rg_last = padded
                n_valid = (ragged.t_off + S0).tolist()
        # the longest option per prompt: its own in list form (the layout is on the host), Lc in tensor form
        longest = lay.lengths.max(1).values.tolist() if continuations is not None else [Lc] * B
        table = self.config.max_position_embeddings
        over = [b for b in range(B) if n_valid[b] + longest[b] > table]
        if over:
            raise ValueError(f"score: prompt(s) {over}: L_b + len = {[n_valid[b] + longest[b] for b in over]} positions are "
                             f"beyond the rotary table (max_position_embeddings = {table})")
        layers = self.model.layers
        H = layers[0].self_attn.num_heads
        hd, dtype = D // H, emb_w.dtype
        if use_cache:
            why = None
            if dtype not in _16BIT:
                why = f"fp32 parameters ({dtype}): the scoring attention takes bf16 / fp16"
            elif not ops.score_attn_ok(dtype, hd, H):
                why = f"ops.score_attn_ok is false for head size {hd} and {H} heads"
            if why is not None:
                raise ValueError(f"score with use_cache=True: {why}; use use_cache=False")

        _dev_check(src)
        if inputs_embeds is None:
            inputs_embeds = ops.embedding_fwd(emb_w, input_ids.long().reshape(-1)).view(B, S0, D)
        fed = lay.fed.to(dev)
        lens = lay.lens.to(dev)
        targets, lengths = lay.targets.to(dev), lay.lengths.to(dev)
        eps = self.model.norm.variance_epsilon
        R = B * n
        own = torch.arange(B, device=dev).repeat_interleave(n)          # the prompt of option row r

        def logprobs(h_rows, ids):    # hidden rows [M, D] -> token_logprobs of ids [M], the logits a bounded chunk at a time
            step = max(1, SCORE_LOGITS_ELEMS // V)
            outs = []
            for r0 in range(0, h_rows.shape[0], step):
                _, y, _ = ops.rmsnorm_fwd(h_rows[r0:r0 + step], self.model.norm.weight, eps)
                outs.append(ops.token_logprobs(ops.linear_fwd(y, self.lm_head.weight), V, ids[r0:r0 + step].contiguous(), m))
            if len(outs) == 1:
                return outs[0]
            return tuple(torch.cat(c) if m or i == 0 else None for i, c in enumerate(zip(*outs)))

        if not use_cache:
            # [prompt | fed tokens] per option, a padded batch: the prompt's mask, then ones over the option's own fed rows
            emb = inputs_embeds.repeat_interleave(n, 0)
            valid = (attention_mask.to(dev) != 0) if attention_mask is not None else torch.ones((B, S0), dtype=torch.bool,
                                                                                                 device=dev)
            col = torch.arange(S0, device=dev)
            last = torch.where(valid, col, torch.full_like(col, -1)).max(1).values           # [B]: the last valid prompt row
            mask = None
            if F:
                emb = torch.cat([emb, ops.embedding_fwd(emb_w, fed).view(R, F, D)], dim=1)
            if F or attention_mask is not None:
                live = torch.arange(F, device=dev) < lens[:, None]                           # [R, F]
                mask = torch.cat([valid.repeat_interleave(n, 0), live], dim=1).to(torch.int32)
            S = S0 + F
            self.model._defer_final_norm = True
            try:
                if mask is not None:
                    h = self.model(inputs_embeds=emb.contiguous(), attention_mask=mask,
                                   position_ids=(mask.cumsum(1) - 1).clamp_(min=0))
                else:
                    h = self.model(inputs_embeds=emb.contiguous())
            finally:
                self.model._defer_final_norm = False
            # the row that predicts token g of option r: the prompt's last valid row for g = 0, fed row g - 1 behind it
            rows = torch.arange(R, device=dev)[:, None] * S + torch.cat(
                [last[own][:, None], S0 + torch.arange(F, device=dev).expand(R, F)], dim=1)
            lp, ti, tl = logprobs(ops.embedding_fwd(h.contiguous().view(R * S, D), rows.reshape(-1).contiguous()),
                                  targets.reshape(-1))
            lp = lp.view(B, n, Lc)
            if m:
                ti, tl = ti.view(B, n, Lc, m), tl.view(B, n, Lc, m)
        else:
            rot = layers[0].self_attn.rotary_emb
            cos, sin = rot.tables(S0 + Lc, dtype, dev)
            if getattr(self, "_lora", None) is not None:      # the per-call merged copies, as in generate()
                from .lora import lora_layers, merged_layer_weights
                merged = dict(merged_layer_weights(self, lyr) for _, lyr in lora_layers(self))
            else:
                merged = {}
            weights = []
            for lyr in layers:
                a, mlp = lyr.self_attn, lyr.mlp
                weights.append(merged.get(lyr) or eng.LayerWeights(
                    a.q_proj.weight, a.k_proj.weight, a.v_proj.weight, a.o_proj.weight, mlp.gate_proj.weight,
                    mlp.up_proj.weight, mlp.down_proj.weight, *lyr.fused_weights()))
            # (1) the prefill, once per prompt at B rows: generate(num_samples=)'s launches
            kvc = [torch.empty((B, S0, 2 * D), dtype=dtype, device=dev) for _ in layers]
            pos = rg_pos if ragged is not None else torch.arange(S0, dtype=torch.int32, device=dev).repeat(B)
            x2 = eng._c2(inputs_embeds, B * S0, D)
            for i, lyr in enumerate(layers):
                ws = weights[i]
                x2 = eng.llama_layer_cached(
                    x2, B, S0, 0, kvc[i], S0, pos, cos, sin, lyr.self_attn.num_heads, lyr.input_layernorm.variance_epsilon,
                    ws.wq, ws.wk, ws.wv, ws.wo, ws.wg, ws.wu, ws.wd, lyr.input_layernorm.weight,
                    lyr.post_attention_layernorm.weight, ws.wqkv, ws.wgu, ragged=ragged)
            # (2) the last valid hidden row of every prompt -> token 0 of each of its options
            if ragged is not None:
                h_last = ops.embedding_fwd(x2.view(B * S0, D), rg_last)
            else:
                h_last = torch.empty((B, D), dtype=dtype, device=dev)
                ops.copy2d(x2, h_last, 1, D, D, D, batch=B, s_src=S0 * D, s_dst=D, src_off=(S0 - 1) * D)
            _, y0, _ = ops.rmsnorm_fwd(h_last, self.model.norm.weight, eps)
            z0 = ops.embedding_fwd(ops.linear_fwd(y0, self.lm_head.weight)[:, :V].contiguous(), own)      # [R, V]
            lp, ti, tl = ops.token_logprobs(z0, V, targets[:, :, 0].reshape(-1).contiguous(), m)
            lp = lp.view(B, n, 1)
            if m:
                ti, tl = ti.view(B, n, 1, m), tl.view(B, n, 1, m)
            if F:
                # (3) the fed rows, one GEMM pass; the tail cache serves one layer at a time
                tail = torch.empty((R, F, 2 * D), dtype=dtype, device=dev)
                t_off = ragged.t_off if ragged is not None else None
                x = ops.embedding_fwd(emb_w, fed)
                for i, lyr in enumerate(layers):
                    x = eng.llama_layer_score(x, B, eng.SharedPrompt(kvc[i], tail, n, S0), lens, t_off, cos, sin,
                                              lyr.self_attn.num_heads, lyr.input_layernorm.variance_epsilon, weights[i],
                                              lyr.input_layernorm.weight, lyr.post_attention_layernorm.weight)
                # (4), (5): fed row (r, g) predicts token g + 1
                lp_f, ti_f, tl_f = logprobs(x, targets[:, :, 1:].reshape(-1))
                lp = torch.cat([lp, lp_f.view(B, n, F)], dim=2)
                if m:
                    ti, tl = torch.cat([ti, ti_f.view(B, n, F, m)], dim=2), torch.cat([tl, tl_f.view(B, n, F, m)], dim=2)
        # behind each option's end: 0.0 / -1 / 0.0, masked on the device
        end = torch.arange(Lc, device=dev) >= lengths[..., None]                             # [B, n, Lc]
        lp = torch.where(end, torch.zeros_like(lp), lp)
        total = torch.zeros((B, n), dtype=torch.float64, device=dev)
        for g in range(Lc):           # the fp64 sum in column order
            total = total + lp[:, :, g].double()
        sums = torch.where(lengths == 0, torch.full_like(total, float("-inf")), total).float()
        if m:
            ti = torch.where(end[..., None], torch.full_like(ti, -1), ti)
            tl = torch.where(end[..., None], torch.zeros_like(tl), tl)
            return ScoreResult(lp, lengths, sums, ti, tl)
        return ScoreResult(lp, lengths, sums, None, None)


# ---------------------------------------------------------- multimodal ------
class MM_LLMs_Config(PretrainedConfig):
    model_type = "mm_llms"
    is_composition = True

    def __init__(self, n_frames=6, attention_heads=8, image_conv_kernel=48, image_conv_stride=36,
                 video_conv_kernel=36, video_conv_stride=30, audio_conv_kernel=240,
                 audio_conv_stride=220, clip_config=None, whisper_config=None, llm_config=None,
                 **kwargs):
        # transformers >= 4.3x instantiates `cls()` with no arguments inside save_pretrained /
        # to_diff_dict; the reference class would raise there.  Default sub-configs keep
        # checkpoint round trips (run_clm_llms_inference.py:455) working.
        clip_config = CLIPConfig() if clip_config is None else clip_config
        whisper_config = WhisperConfig() if whisper_config is None else whisper_config
        llm_config = LlamaConfig() if llm_config is None else llm_config
        for name, sub, klass in (("clip_config", clip_config, CLIPConfig),
                                 ("whisper_config", whisper_config, WhisperConfig),
                                 ("llm_config", llm_config, LlamaConfig)):
            if isinstance(sub, dict):
                sub = klass.from_dict(sub)
                if name == "clip_config":
                    clip_config = sub
                elif name == "whisper_config":
                    whisper_config = sub
                else:
                    llm_config = sub
        self.image_config = clip_config
        self.audio_config = whisper_config
        self.llm_config = llm_config
        self.n_frames = n_frames
        self.attention_heads = attention_heads
        self.image_conv_kernel = image_conv_kernel
        self.image_conv_stride = image_conv_stride
        self.video_conv_kernel = video_conv_kernel
        self.video_conv_stride = video_conv_stride
        self.audio_conv_kernel = audio_conv_kernel
        self.audio_conv_stride = audio_conv_stride
        self.hidden_size = max(llm_config.hidden_size, clip_config.projection_dim,
                               whisper_config.d_model, clip_config.projection_dim)
        super().__init__(**kwargs)

    def to_dict(self):
        output = copy.deepcopy(self.__dict__)
        output["image_config"] = self.image_config.to_dict()
        output["audio_config"] = self.audio_config.to_dict()
        output["llm_config"] = self.llm_config.to_dict()
        for k in ("n_frames", "attention_heads", "image_conv_kernel", "image_conv_stride",
                  "video_conv_kernel", "video_conv_stride", "audio_conv_kernel", "audio_conv_stride",
                  "hidden_size"):
            output[k] = getattr(self, k)
        output["model_type"] = self.__class__.model_type
        return output

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **kwargs):
        config_dict, kwargs = cls.get_config_dict(pretrained_model_name_or_path, **kwargs)
        clip_config = CLIPConfig.from_dict(config_dict["image_config"])
        whisper_config = WhisperConfig.from_dict(config_dict["audio_config"])
        llm_config = LlamaConfig.from_dict(config_dict["llm_config"])
        return cls(clip_config=clip_config, whisper_config=whisper_config, llm_config=llm_config,
                   **kwargs)


def build_prefix_layout(inputs: dict, lq: dict):
    """Integer plumbing of modeling.py:977-1046 (bit-exact by construction, no float math).

    lq maps each PRESENT modality to its number of aligned prefix tokens.  Returns
      ids_full [B,S] int64 : token id at every position of the spliced sequence, -1 where the
                             aligned modal features go.  Final order:
                             [BOS][<image> f.. </image>][<audio> f.. </audio>][<video> f.. </video>][text 1:]
      slots {name: (first feature position, Lq)}
      attention_mask       : ones for the whole prefix PREPENDED to the text mask   (:1036-1040)
      labels               : -100 for the whole prefix PREPENDED to the text labels (:1042-1046)
    Unlike the reference this keeps integer dtypes when no modality is present (the reference's
    empty `torch.tensor([])` is float and breaks the loss; tests/test_oracle.py)."""
    ids = inputs["input_ids"].long()
    B = ids.shape[0]
    cols = [ids[:, :1]]
    slots, pos, ignore = {}, 1, 0
    for name in eng.MODALITIES:
        if name not in lq:
            continue
        n = lq[name]
        cols += [inputs[f"{name}_starts"].long().view(B, 1),
                 torch.full((B, n), -1, dtype=torch.long, device=ids.device),
                 inputs[f"{name}_ends"].long().view(B, 1)]
        slots[name] = (pos + 1, n)
        pos += n + 2
        ignore += n + 2
    cols.append(ids[:, 1:])
    ids_full = torch.cat(cols, dim=1).contiguous()
    attention_mask = labels = None
    if inputs.get("attention_mask") is not None:
        am = inputs["attention_mask"]
        attention_mask = torch.cat([torch.ones((B, ignore), dtype=am.dtype, device=am.device), am], dim=1)
    if inputs.get("labels") is not None:
        lb = inputs["labels"]
        labels = torch.cat([torch.full((B, ignore), -100, dtype=lb.dtype, device=lb.device), lb], dim=1)
    return ids_full, slots, attention_mask, labels


def _mha_params(m: nn.MultiheadAttention):
    return (m.in_proj_weight, m.in_proj_bias, m.bias_k, m.bias_v, m.out_proj.weight, m.out_proj.bias)


class MM_LLMs(PreTrainedModel):
    config_class = MM_LLMs_Config
    supports_gradient_checkpointing = True

    def __init__(self, config):
        super().__init__(config)
        self.config = config
        self.temporal_position_embeddings = nn.Embedding(config.n_frames, config.image_config.projection_dim)
        self.image_encoder = CLIPModel(config.image_config)
        self.video_encoder = CLIPModel(config.image_config)
        self.audio_encoder = WhisperModel(config.audio_config)
        self.llm = LlamaForCausalLM(config.llm_config)
        attn_dropout, kv, za = 0.1, True, True
        pd, D = config.image_config.projection_dim, config.llm_config.hidden_size
        mk = lambda e, h: nn.MultiheadAttention(e, h, dropout=attn_dropout, add_bias_kv=kv,  # noqa: E731
                                                add_zero_attn=za)
        self.temporal_self_attention = mk(pd, config.attention_heads)
        self.video_align_attention = mk(D, config.attention_heads * 2)
        self.audio_align_attention = mk(D, config.attention_heads * 2)
        self.image_align_attention = mk(D, config.attention_heads * 2)
        self.video_long_self_attention = mk(pd, config.attention_heads)
        self.transform_video_to_hidden = nn.Linear(pd, D)
        self.transform_audio_to_hidden = nn.Linear(config.audio_config.d_model, D)
        self.transform_image_to_hidden = nn.Linear(pd, D)
        self.project_image = nn.Conv1d(pd, pd, kernel_size=config.image_conv_kernel,
                                       stride=config.image_conv_stride)
        self.project_video = nn.Conv1d(pd, pd, kernel_size=config.video_conv_kernel,
                                       stride=config.video_conv_stride)
        self.project_audio = nn.Conv1d(config.audio_config.d_model, config.audio_config.d_model,
                                       kernel_size=config.audio_conv_kernel,
                                       stride=config.audio_conv_stride)
        self.logit_scale = nn.Parameter(torch.ones([]) * np.log(1 / 0.07))
        self.layer_norm = nn.LayerNorm(pd)
        self.softmax = nn.Softmax(dim=-1)
        self.relu = nn.ReLU()
        self.gelu = nn.GELU()
        self.elu = nn.ELU()
        self.sigmoid = nn.Sigmoid()
        self.loss_fct = CrossEntropyLoss()
        self._pe_cache = {}
        self._step = 0
        self.dropout_seed = 0x5EED
        self.post_init()

    SEED_STRIDE = 64        # seeds of one step: base + 64 * step + module slot (slot < 64)

    def _dropout_seed(self, slot):
        """seed of dropout site `slot` in training step self._step.  One stride per step, so a step
        replayed from a hipGraph gets the same seeds from base + (device counter += SEED_STRIDE)
        (train.GraphedStep, ops.set_dropout_seed_offset)."""
        return (self.dropout_seed * 1000003 + self._step * self.SEED_STRIDE + slot) & 0x7FFFFFFFFFFF

    # ------------------------------------------------------------ forward ---
    def forward(self, inputs=None):
        _dtype_check(self._param_dtype())
        turn = {}                   # set_session / inputs["session"]: the session arguments of the generate() call
        if inputs.get("session") is not None:
            # a follow-up turn: no tower, no alignment, no bos and no modal prefix -- the text ids as they are, over the
            # session's kept cache
            given = [k for k in ("images", "audios", "videos") if inputs.get(k) is not None]
            if given:
                raise ValueError(f"MM_LLMs.forward: {', '.join(given)} next to inputs['session']: modal rows in a follow-up "
                                 "turn are not built")
            ids = inputs["input_ids"]
            _dev_check(ids)
            E = self.llm.model.embed_tokens.weight
            text_embeddings = ops.embedding_fwd(E, ids.long().reshape(-1)).view(*ids.shape, -1)
            attention_mask, labels = inputs.get("attention_mask"), None
            turn = dict(session=inputs["session"])
        else:
            text_embeddings, attention_mask, labels = self.prepare_inputs_for_generation(inputs)
        if SESSION[0]:
            turn["return_session"] = True
        lora = getattr(self.llm, "_lora", None)
        if lora is not None:        # the adapters' dropout follows this model's step seeds (slot 41)
            lora.ext_seed = self._dropout_seed(lora.SLOT)
        if "inference" in inputs and inputs["inference"] is True:
            # prompt lookup on: the text ids are the lookup history; off: exactly the call without it
            look = dict(input_ids=inputs["input_ids"], **PROMPT_LOOKUP[0]) if PROMPT_LOOKUP[0]["prompt_lookup_num_tokens"] else {}
            # log-probabilities on: the result is GenerateLogprobs; off: exactly the call without them
            lps = LOGPROBS[0] if LOGPROBS[0]["return_logprobs"] else {}
            # guidance on: the negative prompt is the text alone, build_prefix_layout's prompt with no modality, under the
            # text's own mask where the prompt gets its extended one; off: exactly the call without it
            guide = {}
            if GUIDANCE[0] != 1.0:
                ids = inputs["input_ids"].long()
                E = self.llm.model.embed_tokens.weight
                guide = dict(guidance_scale=GUIDANCE[0],
                             negative_inputs_embeds=ops.embedding_fwd(E, ids.reshape(-1)).view(*ids.shape, -1),
                             negative_prompt_attention_mask=inputs.get("attention_mask") if GENERATE_MASK[0] else None)
            # stop sequences / bad words set: passed on; unset: exactly the call without them
            stopping = {k: v for k, v in STOPPING[0].items() if v is not None}
            # parallel samples on: num_samples rows per prompt, the towers and the alignment above run once per prompt;
            # off: exactly the call without it
            par = dict(num_samples=PARALLEL_SAMPLES[0]) if PARALLEL_SAMPLES[0] != 1 else {}
            # adapters set: one name per sample out of the LLM's bank; unset: exactly the call without them
            if ADAPTERS[0] is not None:
                par["adapter_names"] = ADAPTERS[0]
            # a grammar set: every answer is constrained by it; unset: exactly the call without it
            if GRAMMAR[0] is not None:
                par["grammar"] = GRAMMAR[0]
            # a penalty or a bias set: passed on; unset: exactly the call without them
            if PENALTIES[0] != _PENALTIES_OFF:
                par.update(PENALTIES[0])
            # per-request sampling set: one entry per prompt; unset: exactly the call without it
            if SAMPLING_PARAMS[0] is not None:
                par["sampling_params"] = SAMPLING_PARAMS[0]
            # one of the four warpers behind top-p set: passed on; unset: exactly the call without them
            warpers = SAMPLING_WARPERS[0] if SAMPLING_WARPERS[0] != _WARPERS_OFF else {}
            return self.llm.generate(inputs_embeds=text_embeddings, max_new_tokens=128,
                                     eos_token_id=2, bos_token_id=1, pad_token_id=32006,
                                     decode_weights=DECODE_WEIGHTS[0], kv_cache=KV_CACHE[0],
                                     attention_mask=attention_mask if GENERATE_MASK[0] else None, **SAMPLING[0], **warpers,
                                     **lps,
                                     **turn, **guide, **stopping, **par, **BEAM_SEARCH[0], **PROCESSORS[0], **look)
        return self.llm(inputs_embeds=text_embeddings, attention_mask=attention_mask, labels=labels)

    @torch.no_grad()
    def score(self, inputs, continuations=None, **kw):
        """LlamaForCausalLM.score of given answers over the multimodal prompt of `inputs` (forward's dict): the towers and
        the alignment attention run ONCE per prompt (prepare_inputs_for_generation), then llm.score on the embeddings
        with the options of `continuations` (or continuation_ids / continuation_lengths and the other arguments of
        llm.score in kw).  The extended mask is passed under the same switch as inference (set_generate_mask)."""
        _dtype_check(self._param_dtype())
        text_embeddings, attention_mask, _ = self.prepare_inputs_for_generation(inputs)
        return self.llm.score(inputs_embeds=text_embeddings, continuations=continuations,
                              attention_mask=attention_mask if GENERATE_MASK[0] else None, **kw)

    @staticmethod
    def set_fp8(qkv: bool = True, align: bool = True, mlp: bool = False):
        """BASELINE cfg 5: run the forward AND grad-input GEMMs of the fused q|k|v projections
        (modeling.py:159-162) and of the alignment K/V projection of the token table (:882-910) on
        the fp8 MFMA path: e4m3, one scale per token row for activations / gradients, one per
        channel for the weights, which are quantised once per optimizer step (engine.FP8).
        mlp=True extends it to gate|up / down (not part of cfg 5's wording).  Needs bf16
        parameters and fused projections; layers that do not qualify keep the bf16 GEMM.
        Process-wide switch."""
        eng.FP8["qkv"], eng.FP8["align"], eng.FP8["mlp"] = bool(qkv), bool(align), bool(mlp)
        ops.clear_fp8_cache()

    @staticmethod
    def set_decode_weights(mode=None):
        """Weight format of the decode steps of `inputs["inference"] = True` (LlamaForCausalLM.generate's
        decode_weights): None = the 16-bit weights, "fp8" = weight-only e4m3 copies (W8A16: a latency mode, the
        16-bit masters stay resident), "mxfp4" = weight-only MXFP4 copies of the layers' projections and the e4m3
        lm_head (W4A16: likewise a latency mode).  Process-wide switch, like set_fp8."""
        if mode not in (None, "fp8", "mxfp4"):
            raise ValueError(f"set_decode_weights: mode must be None, 'fp8' or 'mxfp4', got {mode!r}")
        DECODE_WEIGHTS[0] = mode

    @staticmethod
    def set_kv_cache(mode=None):
        """KV-cache format of `inputs["inference"] = True` (LlamaForCausalLM.generate's kv_cache): None = 16-bit,
        "fp8" = e4m3 bytes + one fp32 scale per head and position (half the cache's memory and decode traffic;
        composes with set_decode_weights).  Process-wide switch, like set_decode_weights."""
        if mode not in (None, "fp8"):
            raise ValueError(f"set_kv_cache: mode must be None or 'fp8', got {mode!r}")
        KV_CACHE[0] = mode

    @staticmethod
    def set_generate_mask(on=False):
        """Whether `inputs["inference"] = True` passes the extended attention mask it builds (ones for the modal
        prefix, then the text mask) to LlamaForCausalLM.generate (attention_mask=): a padded batch then decodes
        every sample as it would decode alone.  Off by default -- the reference drops the mask at llm.generate
        (modeling.py:959) and attends to the pad tokens.  Process-wide switch, like set_kv_cache."""
        GENERATE_MASK[0] = bool(on)

    @staticmethod
    def set_sampling(do_sample=False, temperature=1.0, top_k=50, top_p=1.0, seed=None, *, min_p=None, typical_p=1.0,
                     epsilon_cutoff=0.0, eta_cutoff=0.0):
        """Token selection of `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the same names):
        greedy by default; do_sample=True draws from the temperature / top-k / top-p filtered distribution, seed=None
        taking a fresh seed from torch's default generator at every call; min_p, typical_p, epsilon_cutoff and eta_cutoff
        (keyword only, off by default) are the four warpers behind top-p.  Validated here when do_sample is set.
        Process-wide switch, like set_decode_weights and set_kv_cache."""
        if do_sample:
            _sampling_check("set_sampling", temperature, top_k, top_p)
            _warpers_check("set_sampling", min_p, typical_p, epsilon_cutoff, eta_cutoff)
        SAMPLING[0] = dict(do_sample=bool(do_sample), temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
        SAMPLING_WARPERS[0] = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)

    @staticmethod
    def set_beam_search(num_beams=1, length_penalty=1.0, early_stopping=False, num_return_sequences=1):
        """Beam search for `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the same names): greedy
        (num_beams=1) by default.  Validated here; what depends on the call (vocabulary, sampling, cache format, mask)
        is validated by generate().  No arguments: back to the default."""
        beam_check("set_beam_search", num_beams, num_return_sequences, length_penalty=length_penalty)
        BEAM_SEARCH[0] = dict(num_beams=int(num_beams), length_penalty=float(length_penalty),
                              early_stopping=bool(early_stopping), num_return_sequences=int(num_return_sequences))

    @staticmethod
    def set_logits_processors(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0):
        """Logits processors for `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the same names):
        off (1.0, 0, 0) by default.  forward passes embeddings only, so the history they look at is the generated
        tokens, as in HF for the reference's call.  Validated here; with beam search on, generate() refuses them.  No
        arguments: back to the default."""
        _processors_check("set_logits_processors", repetition_penalty, no_repeat_ngram_size, min_new_tokens)
        PROCESSORS[0] = dict(repetition_penalty=float(repetition_penalty), no_repeat_ngram_size=int(no_repeat_ngram_size),
                             min_new_tokens=int(min_new_tokens))

    @staticmethod
    def set_prompt_lookup(num_tokens=None, max_matching_ngram_size=2):
        """Prompt-lookup speculative decoding for `inputs["inference"] = True` (LlamaForCausalLM.generate's
        prompt_lookup_num_tokens and max_matching_ngram_size): off (None or 0) by default.  With it on, forward hands its
        text input_ids to generate() as the lookup history.  Validated here; what depends on the call (batch, sampling,
        beams, processors, cache format, mask) is validated by generate().  No arguments: back to the default."""
        G = _lookup_check("set_prompt_lookup", num_tokens, max_matching_ngram_size)
        PROMPT_LOOKUP[0] = dict(prompt_lookup_num_tokens=G or None, max_matching_ngram_size=int(max_matching_ngram_size))

    @staticmethod
    def set_logprobs(return_logprobs=False, top_logprobs=0):
        """Token log-probabilities for `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the same
        names): off by default.  With return_logprobs=True forward returns GenerateLogprobs(ids, logprobs, top_ids,
        top_logprobs) in place of the ids, top_logprobs=n in [1, 20] adding the n most likely columns of every step.
        Validated here; what depends on the call (beams, prompt lookup) is validated by generate().  No arguments: back
        to off.  Process-wide switch, like set_sampling."""
        _logprobs_check("set_logprobs", return_logprobs, top_logprobs)
        LOGPROBS[0] = dict(return_logprobs=bool(return_logprobs), top_logprobs=int(top_logprobs))

    @staticmethod
    def set_guidance(guidance_scale=1.0):
        """Classifier-free guidance for `inputs["inference"] = True` (LlamaForCausalLM.generate's guidance_scale): off
        (1.0) by default.  With it on, forward hands generate() the embedding of its text input_ids alone -- the prompt
        without the image, audio or video rows -- as negative_inputs_embeds, so every step is steered towards what the
        modal input adds; with set_generate_mask(True) the text's attention mask goes with it.  Validated here; what
        depends on the call (beams, prompt lookup, dtype) is validated by generate().  No arguments: back to off.
        Process-wide switch, like set_sampling."""
        s = _guidance_check("set_guidance", guidance_scale)
        GUIDANCE[0] = 1.0 if s is None else s

    @staticmethod
    def set_stopping(stop_sequences=None, bad_words_ids=None):
        """Stop sequences and banned words for `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the
        same names): both off (None) by default.  forward passes embeddings only, so the history the banned words look at
        is the generated tokens; a banned [2] is the call's eos and is dropped.  Validated here; what depends on the call
        (beams, prompt lookup) is validated by generate().  No arguments: back to off.  Process-wide switch, like
        set_logits_processors."""
        _stopping_check("set_stopping", stop_sequences, bad_words_ids)
        STOPPING[0] = dict(stop_sequences=None if stop_sequences is None else [list(q) for q in stop_sequences],
                           bad_words_ids=None if bad_words_ids is None else [list(q) for q in bad_words_ids])

    @staticmethod
    def set_session(on=False):
        """Multi-turn sessions for `inputs["inference"] = True` (LlamaForCausalLM.generate's return_session): off by
        default.  With it on forward returns (result, session); `inputs["session"] = s` then continues s -- forward runs
        no tower and no alignment, embeds inputs["input_ids"] as they are (no bos, no modal prefix), passes
        inputs.get("attention_mask") under set_generate_mask as a first call does, and updates s in place.  images, audios
        or videos next to a session raise ValueError (modal rows in a follow-up turn are not built).  What depends on the
        call (beams, parallel samples, prompt lookup, guidance, cache format, dtype) is validated by generate().
        Process-wide switch, like set_generate_mask."""
        SESSION[0] = bool(on)

    @staticmethod
    def set_adapters(names=None):
        """Mixed-adapter LoRA for `inputs["inference"] = True` (LlamaForCausalLM.generate's adapter_names): off (None) by
        default.  names: one adapter name per sample out of the LLM's lora.AdapterBank (`AdapterBank(model.llm)`),
        "__base__" for none.  Only the form is validated here (a list / tuple of str); the names, their count and what the
        call composes with are validated by generate().  No arguments: back to off.  Process-wide switch, like
        set_parallel_samples."""
        if names is not None:
            if isinstance(names, str) or not isinstance(names, (list, tuple)) or not all(isinstance(n, str) for n in names):
                raise ValueError(f"set_adapters: names must be None or a list of adapter names (str), got {names!r}")
            names = list(names)
        ADAPTERS[0] = names

    @staticmethod
    def set_grammar(g=None):
        """Grammar-constrained decoding for `inputs["inference"] = True` (LlamaForCausalLM.generate's grammar): off (None)
        by default.  g: a grammar.TokenDFA applied to every sample, or a list with one TokenDFA | None per sample.  With a
        LLaMA SentencePiece tokenizer, grammar.vocab_bytes(tokenizer.convert_ids_to_tokens(range(V)), special ids) is the
        vocabulary TokenDFA.from_regex takes.  The form is validated here; what depends on the call (beams, prompt lookup,
        sessions, the batch, the vocabulary size) is validated by generate().  No arguments: back to off.  Process-wide
        switch, like set_stopping."""
        if g is not None:
            g = _grammar_check("set_grammar", g)
        GRAMMAR[0] = g

    @staticmethod
    def set_penalties(frequency_penalty=0.0, presence_penalty=0.0, logit_bias=None):
        """The per-request penalties for `inputs["inference"] = True` (LlamaForCausalLM.generate's arguments of the same
        names): off (0.0, 0.0, None) by default.  Each penalty is a float or one float per sample, logit_bias a dict
        {token id: bias} for every sample or a list with one dict | None per sample.  The form and the ranges are
        validated here; what depends on the call (the batch, the vocabulary size, beams, prompt lookup) is validated by
        generate().  No arguments: back to off.  Process-wide switch, like set_logits_processors."""
        frequency_penalty, presence_penalty = (v.detach().cpu().tolist() if isinstance(v, torch.Tensor) else v
                                               for v in (frequency_penalty, presence_penalty))
        _penalties_check("set_penalties", frequency_penalty, presence_penalty, logit_bias)
        PENALTIES[0] = dict(frequency_penalty=frequency_penalty, presence_penalty=presence_penalty, logit_bias=logit_bias)

    @staticmethod
    def set_sampling_params(params=None):
        """Per-request sampling for `inputs["inference"] = True` (LlamaForCausalLM.generate's sampling_params): off (None)
        by default.  params: a list with one entry per prompt, each None (greedy) or a dict out of temperature, top_k,
        top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff and seed.  The form and the values are validated here; what
        depends on the call (the batch, set_sampling(do_sample=True) next to it, beams, prompt lookup, parallel samples)
        is validated by generate().  No argument: back to off.  Process-wide switch, like set_penalties."""
        if params is not None:
            _sampling_params_check("set_sampling_params", params)
            params = [None if e is None else dict(e) for e in params]
        SAMPLING_PARAMS[0] = params

    @staticmethod
    def set_parallel_samples(num_samples=1):
        """Parallel sampling for `inputs["inference"] = True` (LlamaForCausalLM.generate's num_samples): off (1) by default.
        With n > 1 forward returns ids [B * n, width], row b * n + j sample j of prompt b; the towers, the alignment and
        the prefill run once per prompt.  It needs set_sampling(do_sample=True).  Validated here; what depends on the
        call (sampling, beams, prompt lookup, guidance, cache format, dtype) is validated by generate().  No arguments:
        back to off.  Process-wide switch, like set_logprobs."""
        PARALLEL_SAMPLES[0] = _num_samples_check("set_parallel_samples", num_samples)

    def prepare_inputs_for_generation(self, inputs):
        """modeling.py:965-1048 — same outputs (inputs_embeds, attention_mask, labels)."""
        cfg = self.config
        audio_f, audio_side = None, None
        if inputs.get("audios") is not None:
            # The towers are independent of each other: with frozen encoders (run_clm_llms.py:390-393) the audio tower
            # goes out on a second stream beside the image / video tower (engine.ENC_SIDE; their short-K GEMMs and 4-wave
            # attention leave CUs idle between rounds: +0.4 % of the cfg-3 step)
            audio_side = eng.tower_side_stream(inputs["audios"], self.audio_encoder,
                                               other=inputs.get("images") is not None or inputs.get("videos") is not None)
            if audio_side is not None:
                audio_side.wait_stream(torch.cuda.current_stream(inputs["audios"].device))
                with torch.cuda.stream(audio_side):
                    audio_f = self.encode_audio(inputs["audios"])
            else:
                audio_f = self.encode_audio(inputs["audios"])
        image_f = self.encode_image(inputs["images"]) if inputs.get("images") is not None else None
        video_f = self.encode_video_long(inputs["videos"]) if inputs.get("videos") is not None else None
        if audio_side is not None:
            main = torch.cuda.current_stream(audio_f.device)
            main.wait_stream(audio_side)
            audio_f.record_stream(main)
        E = self.llm.model.embed_tokens.weight
        ids = inputs["input_ids"]
        _dev_check(ids)
        ids = ids.long()
        B, L = ids.shape
        feats = dict(image=image_f, audio=audio_f, video=video_f)
        geom = dict(image=(cfg.image_conv_kernel, cfg.image_conv_stride),
                    audio=(cfg.audio_conv_kernel, cfg.audio_conv_stride),
                    video=(cfg.video_conv_kernel, cfg.video_conv_stride))
        lq = {}
        for name in eng.MODALITIES:
            if feats[name] is not None:
                kw, st = geom[name]
                lq[name] = (feats[name].shape[1] - kw) // st + 1
        ids_full, slots, attention_mask, labels = build_prefix_layout(inputs, lq)
        self._step += 1
        p = 0.1 if self.training else 0.0
        meta = dict(ids_full=ids_full, slots=slots, heads=cfg.attention_heads * 2, geom=geom, p=p,
                    seeds={n: self._dropout_seed(i) for i, n in enumerate(eng.MODALITIES)},
                    padding_idx=-1 if self.llm.model.padding_idx is None else self.llm.model.padding_idx)
        params = []
        for name in eng.MODALITIES:
            conv = getattr(self, f"project_{name}")
            lin = getattr(self, f"transform_{name}_to_hidden")
            params += [conv.weight, conv.bias, lin.weight, lin.bias,
                       *_mha_params(getattr(self, f"{name}_align_attention"))]
        text_embeddings = eng.PrefixAssembleFn.apply(E, meta, image_f, audio_f, video_f, *params)

        return text_embeddings, attention_mask, labels

    # ----------------------------------------------------------- encoders ---
    def _param_dtype(self):
        return self.llm.model.embed_tokens.weight.dtype

    def _clip_tokens(self, clip: CLIPModel, images):
        """visual_projection(vision_model(x)[0])[:, 1:, :]  (modeling.py:1073,1092)."""
        _dev_check(images)
        vm = clip.vision_model
        vcfg = clip.config.vision_config
        dtype = vm.embeddings.patch_embedding.weight.dtype
        x = ops.cast(images.contiguous(), dtype)
        B = x.shape[0]
        P, Ed = vcfg.patch_size, vcfg.hidden_size
        g = vcfg.image_size // P
        T = g * g + 1
        if x.shape[-1] != vcfg.image_size or x.shape[-2] != vcfg.image_size:
            raise ValueError(f"Input image size ({x.shape[-2]}*{x.shape[-1]}) doesn't match model "
                             f"({vcfg.image_size}*{vcfg.image_size}).")
        h = eng.ClipEmbedFn.apply(x, vm.embeddings.patch_embedding.weight,
                                  vm.embeddings.class_embedding,
                                  vm.embeddings.position_embedding.weight, P)
        h = eng.LayerNormFn.apply(h, vm.pre_layrnorm.weight, vm.pre_layrnorm.bias, vcfg.layer_norm_eps)
        act = eng.ACT_CODE[vcfg.hidden_act]
        for lyr in vm.encoder.layers:
            a, m = lyr.self_attn, lyr.mlp
            h = eng.EncoderLayerFn.apply(
                h, vcfg.num_attention_heads, vcfg.layer_norm_eps, act, lyr.layer_norm1.weight,
                lyr.layer_norm1.bias, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.k_proj.bias,
                a.v_proj.weight, a.v_proj.bias, a.out_proj.weight, a.out_proj.bias,
                lyr.layer_norm2.weight, lyr.layer_norm2.bias, m.fc1.weight, m.fc1.bias, m.fc2.weight,
                m.fc2.bias, *fused_encoder_qkv(a))
        return eng.DropClsProjectFn.apply(h, clip.visual_projection.weight)

    def encode_image(self, images):
        return self._clip_tokens(self.image_encoder, images)

    def encode_audio(self, audios):
        """audio_encoder.encoder(audios)[0]  (modeling.py:1081-1083)."""
        _dev_check(audios)
        enc = self.audio_encoder.encoder
        wcfg = self.audio_encoder.config
        dtype = enc.conv1.weight.dtype
        x = ops.cast(audios.contiguous(), dtype)
        expected = wcfg.max_source_positions * 2
        if x.shape[-1] != expected:
            raise ValueError(f"Whisper expects the mel input features to be of length {expected}, "
                             f"but found {x.shape[-1]}.")
        h = eng.WhisperStemFn.apply(x, enc.conv1.weight, enc.conv1.bias, enc.conv2.weight,
                                    enc.conv2.bias, enc.embed_positions.weight)
        act = eng.ACT_CODE[wcfg.activation_function]
        for lyr in enc.layers:
            a = lyr.self_attn
            h = eng.EncoderLayerFn.apply(
                h, wcfg.encoder_attention_heads, 1e-5, act, lyr.self_attn_layer_norm.weight,
                lyr.self_attn_layer_norm.bias, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, None,
                a.v_proj.weight, a.v_proj.bias, a.out_proj.weight, a.out_proj.bias,
                lyr.final_layer_norm.weight, lyr.final_layer_norm.bias, lyr.fc1.weight, lyr.fc1.bias,
                lyr.fc2.weight, lyr.fc2.bias, *fused_encoder_qkv(a))
        return eng.LayerNormFn.apply(h, enc.layer_norm.weight, enc.layer_norm.bias, 1e-5)

    def encode_video_long(self, videos):
        """modeling.py:1070-1079."""
        _dev_check(videos)
        nf = self.config.n_frames
        frames = videos.reshape(-1, videos.size(-3), videos.size(-2), videos.size(-1))
        f = self._clip_tokens(self.video_encoder, frames)           # [B*nf, T, pd]
        Bv = frames.size(0) // nf
        f = f.reshape(Bv, nf * f.size(1), f.size(2))
        pe = self._positional_encoding(f.size(1), f.size(2), f.dtype, f.device)
        f = eng.AddBroadcastFn.apply(f, pe)
        m = self.video_long_self_attention
        p = m.dropout if self.training else 0.0
        return eng.MHASelfFn.apply(f, m.num_heads, p, self._dropout_seed(40), *_mha_params(m))

    def _positional_encoding(self, L, h, dtype, device):
        """create_positional_encoding (modeling.py:1095-1106) is input independent: built once
        per (L, h) instead of by a 590k-iteration Python loop every forward."""
        key = (L, h, dtype, str(device))
        if key not in self._pe_cache:
            self._pe_cache[key] = ops.cast(create_positional_encoding(L, h).to(device), dtype)
        return self._pe_cache[key]

    def encode_video(self, videos):
        raise NotImplementedError("encode_video is dead code in the reference (modeling.py:969 uses "
                                  "encode_video_long); not on the hot path")


def create_positional_encoding(L, h):
    """modeling.py:1095-1106, vectorised (the reference fills the [L, h] table with a Python double loop):
    pe[pos, i] = sin(pos * w_i), pe[pos, i + 1] = cos(pos * w_i), w_i = exp(-(ln 10000 / h) * 2 i) for EVEN i --
    the reference's exponent uses 2 i with i already stepping by 2, kept as it is.  fp32 on
    the CPU like the reference's; pinned to it by tests/test_oracle.py::test_reference_positional_encoding."""
    i = torch.arange(0, h, 2, dtype=torch.float32)
    div = torch.exp(-(math.log(10000.0) / h * (2 * i)))
    posn = torch.arange(L, dtype=torch.float32)[:, None]
    pe = torch.zeros(L, h)
    pe[:, 0::2] = torch.sin(posn * div)
    pe[:, 1::2] = torch.cos(posn * div)
    return pe


def add_positional_encoding(tensor):
    """modeling.py:1108-1118 on the device path."""
    N, L, h = tensor.size()
    pe = create_positional_encoding(L, h)
    return eng.AddBroadcastFn.apply(tensor, ops.cast(pe.to(tensor.device), tensor.dtype))
