"""CPU: per-request sampling, generate(sampling_params=[...]) -- the argument's validation and normalisation, the
restatement of the per-row table (tests/sampling_params_ref.py) against the restatements of the scalar rules, the record
ops.SampleTable writes, the seeds, the ABI of the two new entries and the resources of their kernels."""
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import sampling_params_ref as R
from test_sampling_cpu import greedy, sample_row, uniform
from warpers_ref import logits_host, warp_row

from macaw_llm_amd import lib as L
from macaw_llm_amd import modeling as Mo
from macaw_llm_amd import ops

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
NAN, INF = float("nan"), float("inf")
KEYS = ("temperature", "top_k", "top_p", "min_p", "typical_p", "epsilon_cutoff", "eta_cutoff", "seed")


class _PastTheChecks(Exception):
    pass


class _NoModel:
    """generate() validates its arguments before it touches the model: reaching the model means nothing was refused"""

    def __getattr__(self, name):
        raise _PastTheChecks(name)


def _generate(B=2, **kw):
    return Mo.LlamaForCausalLM.generate(_NoModel(), inputs_embeds=torch.zeros(B, 2, 4, dtype=torch.bfloat16), **kw)


# ------------------------------------------------------------------------------------------------ 1. validation --
def test_every_refusal_is_a_value_error_that_names_the_condition_before_the_model_is_touched():
    d = dict(temperature=0.8, top_k=5, seed=1)
    with pytest.raises(ValueError, match=r"sampling_params=\) with do_sample=True: two ways"):
        _generate(sampling_params=[d, None], do_sample=True)
    for bad in ({"temperature": 1.0}, "greedy", 3, torch.zeros(2)):
        with pytest.raises(ValueError, match=rf"sampling_params must be None or a list .* got {type(bad).__name__}"):
            _generate(sampling_params=bad)
    for bad in ([], [d], [d, None, d], (None,)):
        with pytest.raises(ValueError, match=rf"sampling_params holds {len(bad)} entries for 2 prompts"):
            _generate(sampling_params=bad)
    for bad in (0.7, "x", [d], (1, 2), True):
        with pytest.raises(ValueError, match=rf"generate: sampling_params\[1\] must be None or a dict, got "
                                             rf"{type(bad).__name__}"):
            _generate(sampling_params=[None, bad])
    for key in ("do_sample", "stream", "max_new_tokens", "repetition_penalty", 3):
        with pytest.raises(ValueError, match=rf"generate: sampling_params\[0\]: unknown key {key!r}; the keys are "
                                             "temperature, top_k, top_p, min_p, typical_p, epsilon_cutoff, eta_cutoff, seed"):
            _generate(sampling_params=[{key: 1}, None])
    # a bad value: the scalar rules' own messages behind the entry's name
    with pytest.raises(ValueError) as e:
        _generate(sampling_params=[None, dict(top_p=1.5)])
    assert str(e.value) == "generate: sampling_params[1]: top_p must lie in (0, 1], got 1.5"
    for bad, msg in ((dict(temperature=-1.0), "temperature must be a finite number > 0, got -1.0"),
                     (dict(temperature=INF), "temperature must be a finite number > 0"),
                     (dict(temperature=NAN), "temperature must be a finite number > 0"),
                     (dict(temperature="1"), "temperature must be a finite number > 0"),
                     (dict(top_p=0.0), r"top_p must lie in \(0, 1\], got 0.0"),
                     (dict(top_k=-1), "top_k must be None or an integer >= 0, got -1"),
                     (dict(top_k=2.5), "top_k must be None or an integer >= 0"),
                     (dict(min_p=1.5), r"min_p must be None or lie in \[0, 1\], got 1.5"),
                     (dict(typical_p=0.0), r"typical_p must lie in \(0, 1\], got 0.0"),
                     (dict(epsilon_cutoff=1.0), r"epsilon_cutoff must lie in \[0, 1\), got 1.0"),
                     (dict(eta_cutoff=-0.1), r"eta_cutoff must lie in \[0, 1\), got -0.1"),
                     (dict(seed=1.5), "seed must be None or an integer, got 1.5"),
                     (dict(seed="7"), "seed must be None or an integer"),
                     (dict(seed=True), "seed must be None or an integer"),
                     # a greedy entry's other keys are validated all the same
                     (dict(temperature=0, top_p=2.0), r"top_p must lie in \(0, 1\], got 2.0"),
                     (dict(temperature=0.0, min_p=-1), "min_p must be None or lie")):
        with pytest.raises(ValueError, match=r"generate: sampling_params\[1\]: " + msg):
            _generate(sampling_params=[d, bad])
        with pytest.raises(ValueError, match=r"set_sampling_params: sampling_params\[0\]: " + msg):
            Mo.MM_LLMs.set_sampling_params([bad])
    assert Mo.SAMPLING_PARAMS[0] is None                                  # a refused call changes nothing
    with pytest.raises(ValueError, match=r"sampling_params=\) with num_beams=2: per-request sampling along beams is not "
                                         "built"):
        _generate(sampling_params=[d, None], num_beams=2)
    with pytest.raises(ValueError, match=r"sampling_params=\) with prompt_lookup_num_tokens=4: .* not built"):
        _generate(sampling_params=[d, None], prompt_lookup_num_tokens=4)
    for rows in ([d, None], [None, None], [d, dict(temperature=0)]):
        with pytest.raises(ValueError, match=r"generate\(num_samples=3\) with a greedy entry in sampling_params \(entry "
                                             rf"{[r is None or r.get('temperature') == 0 for r in rows].index(True)}\).*"
                                             "3 identical rows"):
            _generate(sampling_params=rows, num_samples=3)
    # what passes: to the model
    for ok in ([d, None], (None, d), [None, None], [{}, {}], [dict(temperature=0), dict(top_k=None, min_p=None)],
               [dict(zip(KEYS, (0.7, 40, 0.9, 0.05, 0.9, 1e-3, 2e-3, 2 ** 64 - 1))), dict(seed=-5)]):
        with pytest.raises(_PastTheChecks):
            _generate(sampling_params=ok)
    with pytest.raises(_PastTheChecks):
        _generate(sampling_params=[d, dict(temperature=2.0)], num_samples=3)


def test_the_scalar_arguments_keep_their_behaviour_and_their_messages():
    with pytest.raises(ValueError, match="generate: temperature must be a finite number > 0, got 0.0"):
        _generate(do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match=r"prompt_lookup_num_tokens=4\): do_sample=True"):
        _generate(do_sample=True, prompt_lookup_num_tokens=4)
    with pytest.raises(ValueError, match=r"num_samples=2\) with do_sample=False: greedy decoding would return 2 identical"):
        _generate(num_samples=2)
    with pytest.raises(_PastTheChecks):
        _generate(temperature=0.0)                                        # ignored by greedy decoding, as before


# -------------------------------------------------------------------------------------------------- 2. defaults --
def test_generate_and_set_sampling_params_carry_the_argument():
    p = inspect.signature(Mo.LlamaForCausalLM.generate).parameters
    assert p["sampling_params"].default is None
    p = inspect.signature(Mo.MM_LLMs.set_sampling_params).parameters
    assert list(p) == ["params"] and p["params"].default is None
    assert Mo.SAMPLING_PARAMS[0] is None
    try:
        rows = [dict(temperature=0.5, seed=3), None]
        Mo.MM_LLMs.set_sampling_params(rows)
        assert Mo.SAMPLING_PARAMS[0] == rows and Mo.SAMPLING_PARAMS[0][0] is not rows[0]      # its own copy
        Mo.MM_LLMs.set_sampling_params()
        assert Mo.SAMPLING_PARAMS[0] is None
    finally:
        Mo.SAMPLING_PARAMS[0] = None
    fwd = inspect.getsource(Mo.MM_LLMs.forward)
    assert 'par["sampling_params"] = SAMPLING_PARAMS[0]' in fwd and "SAMPLING_PARAMS[0] is not None" in fwd
    doc = Mo.LlamaForCausalLM.generate.__doc__
    for phrase in ("sampling_params=[...]", "never on its place in the batch", "the SELECTION is position-independent",
                   "Out of scope: per-row max_new_tokens"):
        assert phrase in doc, phrase
    assert tuple(Mo._SAMPLING_PARAMS_DEFAULTS) == KEYS
    sig = inspect.signature(Mo.LlamaForCausalLM.generate).parameters    # a missing key takes generate()'s own default
    assert {k: sig[k].default for k in KEYS} == Mo._SAMPLING_PARAMS_DEFAULTS


def test_entries_normalise_to_greedy_or_to_the_scalar_calls_values():
    chk = Mo._sampling_params_check
    assert chk("generate", [None, None, None], 3) == [None, None, None]
    assert chk("generate", [dict(temperature=0), dict(temperature=0.0, top_k=3, seed=9)]) == [None, None]
    got = chk("generate", [{}, dict(temperature=2, top_k=None, top_p=0.5, min_p=0.1, seed=-1)], 2)
    assert got[0] == dict(temperature=1.0, top_k=50, top_p=1.0, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0,
                          eta_cutoff=0.0, seed=None)
    assert got[1] == dict(temperature=2.0, top_k=0, top_p=0.5, min_p=0.1, typical_p=1.0, epsilon_cutoff=0.0,
                          eta_cutoff=0.0, seed=-1)
    # what the scalar call hands to its launch, value for value
    for d in (dict(temperature=0.7, top_k=40, top_p=0.9), dict(min_p=0.05, typical_p=0.9, eta_cutoff=1e-3)):
        v = {**Mo._SAMPLING_PARAMS_DEFAULTS, **d}
        r = chk("generate", [d])[0]
        assert (r["temperature"], r["top_k"], r["top_p"]) == Mo._sampling_check("x", v["temperature"], v["top_k"], v["top_p"])
        w = Mo._warpers_check("x", v["min_p"], v["typical_p"], v["epsilon_cutoff"], v["eta_cutoff"]) or (0.0, 1.0, 0.0, 0.0)
        assert (r["min_p"], r["typical_p"], r["epsilon_cutoff"], r["eta_cutoff"]) == w


def test_num_samples_expansion_gives_row_b_n_plus_j_stream_j():
    rows = Mo._sampling_params_check("generate", [dict(temperature=0.5, seed=11), None, dict(top_k=2 ** 40, seed=12)])
    out = Mo._sampling_params_rows(rows, 3)
    assert len(out) == 9 and out[3:6] == [None, None, None]
    for b, seed, T in ((0, 11, 0.5), (2, 12, 1.0)):
        for j in range(3):
            r = out[b * 3 + j]
            assert (r["stream"], r["seed"], r["temperature"]) == (j, seed, T)
    assert out[6]["top_k"] == 2 ** 31 - 1                               # at or above any vocabulary: off, and an int32
    assert [r["stream"] for r in Mo._sampling_params_rows(rows[:1], 1)] == [0]
    t = ops.SampleTable(out, "cpu")
    assert t.rows == 9 and t.sampled == [True] * 3 + [False] * 3 + [True] * 3


def test_seed_none_draws_distinct_seeds_in_prompt_order_that_repeat_after_manual_seed():
    rows = Mo._sampling_params_check("generate", [dict(), None, dict(seed=5), dict(temperature=0.3), dict(temperature=0)])
    torch.manual_seed(77)
    a = Mo._sampling_params_rows(rows, 2)
    after = torch.randint(0, 10 ** 9, (1,)).item()
    seeds = [r["seed"] for r in a if r is not None]
    assert seeds[0] == seeds[1] and seeds[2] == seeds[3] == 5 and seeds[4] == seeds[5]      # one seed per prompt
    assert seeds[0] != seeds[4] and all(0 <= s < 2 ** 63 for s in seeds)
    torch.manual_seed(77)
    assert Mo._sampling_params_rows(rows, 2) == a
    assert Mo._sampling_params_rows(rows, 2) != a                        # the generator has moved on
    # exactly one draw per sampled prompt without a seed, none for a greedy or a seeded one: the scalar call's draws
    torch.manual_seed(77)
    want = [int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64)) for _ in range(2)]
    assert [seeds[0], seeds[4]] == want and torch.randint(0, 10 ** 9, (1,)).item() == after
    assert rows[0]["seed"] is None                                       # the checked entries are not written to


# -------------------------------------------------------------------------------------------- 3. the restatement --
RECS = [None,
        dict(temperature=0.7, top_k=5, seed=101, stream=3),
        dict(top_p=0.9, seed=102, stream=1),
        dict(temperature=0.8, top_k=40, top_p=0.95, min_p=0.02, typical_p=0.9, epsilon_cutoff=1e-3, eta_cutoff=2e-3,
             seed=2 ** 63 + 5, stream=7),
        dict(top_k=10 ** 6, seed=104, stream=0),
        dict(temperature=0.3, seed=105, stream=2 ** 32 - 1)]


def test_a_sampled_row_is_the_scalar_restatement_at_row_stream_and_a_greedy_row_is_greedy():
    V = 300
    _, xh = logits_host(V, len(RECS), V + 4, 3.0, "bf16")
    assert [R.form(r) for r in RECS] == ["greedy", "sample", "sample", "warp", "sample", "sample"]
    for step in (0, 9):
        got = R.table_rows(xh, V, RECS, step)
        assert got[0] == greedy(xh[0]) == int(np.argmax(xh[0]))
        for i in (1, 2, 4, 5):
            r = R.full(RECS[i])
            assert got[i] == sample_row(xh[i], V, r["temperature"], r["top_k"], r["top_p"], r["seed"], step, row=r["stream"])
        r = R.full(RECS[3])
        w = warp_row(xh[3], V, r["temperature"], r["top_k"], r["top_p"], *R.warpers(r))
        kept = np.nonzero(w["kept"])[0]
        cum = np.cumsum(w["e"][kept])
        assert got[3] == int(kept[np.nonzero(cum > uniform(r["seed"], step, r["stream"]) * cum[-1])[0][0]])
        # the place in the batch is no argument: any order of the rows gives the same tokens
        perm = [4, 0, 5, 3, 1, 2]
        assert R.table_rows(xh[perm], V, [RECS[i] for i in perm], step) == [got[i] for i in perm]
    # with every warper off the warp form IS the plain one
    r = dict(RECS[1], min_p=0.0, typical_p=1.0)
    assert R.form(r) == "sample" and R.table_row(xh[1], V, r, 4) == R.table_row(xh[1], V, RECS[1], 4)
    # seed, stream and step all reach the draw
    hot = dict(temperature=5.0, seed=1, stream=0)
    base = [R.table_row(xh[2], V, hot, s) for s in range(8)]
    assert base != [R.table_row(xh[2], V, dict(hot, seed=2), s) for s in range(8)]
    assert base != [R.table_row(xh[2], V, dict(hot, stream=1), s) for s in range(8)]
    assert len(set(base)) > 1


def test_special_rows_and_records_outside_the_domain():
    tie = np.array([1.0, 7.0, 3.0, 7.0, 0.0], dtype=np.float32)
    bad = np.array([np.nan, -np.inf, 0.5, np.nan, 0.25, -np.inf], dtype=np.float32)
    ninf = np.full(4, -np.inf, dtype=np.float32)
    assert R.table_row(tie, 5, None) == 1 and R.table_row(bad, 6, None) == 0 and R.table_row(ninf, 4, None) == 0
    rec = dict(temperature=1.0, top_k=0, seed=3)
    assert {R.table_row(bad, 6, rec, s) for s in range(100)} == {2, 4}   # NaN and -inf are never drawn
    assert R.table_row(ninf, 4, rec) == 0 and R.table_row(ninf, 4, dict(rec, min_p=0.1)) == 0
    assert {R.table_row(tie, 5, dict(rec, top_k=1), s) for s in range(20)} == {1}
    for out in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=NAN), dict(temperature=INF),
                dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(min_p=2.0), dict(typical_p=0.0),
                dict(epsilon_cutoff=1.0), dict(eta_cutoff=-0.5), dict(mode=2), dict(mode=0)):
        assert R.form(dict(rec, **out)) == "greedy", out
        assert R.table_row(tie, 5, dict(rec, **out), 3) == 1


def test_sample_table_writes_the_headers_record():
    assert R.RECORD.size == ops.SampleTable.RECORD.size == 48 and R.RECORD.format == ops.SampleTable.RECORD.format
    t = ops.SampleTable(RECS, "cpu")
    assert t.records.dtype == torch.uint8 and tuple(t.records.shape) == (len(RECS), 48) and t.records.is_contiguous()
    assert t.rows == len(RECS) and t.sampled == [r is not None for r in RECS]
    raw = t.records.numpy().tobytes()
    assert raw == b"".join(R.pack(r) for r in RECS)
    u = R.unpack(raw[3 * 48:4 * 48])
    assert (u["seed"], u["stream"], u["mode"], u["top_k"]) == (2 ** 63 + 5, 7, 1, 40)
    assert u["temperature"] == np.float32(0.8) and u["eta_cutoff"] == np.float32(2e-3)
    g = R.unpack(raw[:48])
    assert g["mode"] == 0 and g["temperature"] == 1.0
    # the layout the header states, byte for byte
    src = open(HEADER).read()
    rule = src[src.index("Per-row sampling table"):src.index("int mk_sample_rows_table(")]
    offs = {name: int(m) for m, name in re.findall(r"byte +(\d+) +\w+ +(\w+)", rule)}
    assert offs == dict(temperature=0, top_k=4, top_p=8, min_p=12, typical_p=16, epsilon_cutoff=20, eta_cutoff=24,
                        stream=28, seed=32, mode=40, reserved=44)
    one = ops.SampleTable([dict(temperature=0.5, top_k=3, top_p=0.25, min_p=0.125, typical_p=0.75, epsilon_cutoff=0.0625,
                                eta_cutoff=0.03125, seed=0x0102030405060708, stream=0x0A0B0C0D)], "cpu").records[0]
    f32 = one[:28].view(torch.float32).tolist()
    assert [f32[0]] + f32[2:] == [0.5, 0.25, 0.125, 0.75, 0.0625, 0.03125]
    assert one[4:8].view(torch.int32).item() == 3 and one[28:32].tolist() == [0x0D, 0x0C, 0x0B, 0x0A]
    assert one[32:40].tolist() == [8, 7, 6, 5, 4, 3, 2, 1] and one[40:].view(torch.int32).tolist() == [1, 0]
    for bad in ([], [dict(temperature=0.0)], [dict(top_p=1.5)], [dict(top_k=-1)], [dict(min_p=2.0)], [dict(stream=-1)],
                [dict(stream=2 ** 32)], [dict(seed=1.5)], [dict(do_sample=True)], [[0.7]], [dict(temperature=NAN)]):
        with pytest.raises(L.MacawHipError, match="SampleTable"):
            ops.SampleTable(bad, "cpu")


def test_the_wrappers_check_the_table_against_the_logits():
    x = torch.zeros((3, 8))
    t = ops.SampleTable([None, None], "cpu")
    with pytest.raises(L.MacawHipError, match="a SampleTable of 2 rows for logits"):
        ops.sample_rows_table(x, 8, t)
    with pytest.raises(L.MacawHipError, match="a SampleTable of 2 rows for logits"):
        ops.decode_emit_sample_table(x, 8, 0, 2, None, None, None, None, t)
    with pytest.raises(L.MacawHipError, match="table must be an ops.SampleTable"):
        ops.sample_rows_table(x, 8, [None] * 3)


# ------------------------------------------------------------------------------------------------------ 4. ABI --
def test_header_declares_the_two_entries_and_states_the_rule():
    src = open(HEADER).read()
    for name, n in (("mk_sample_rows_table", 9), ("mk_decode_emit_sample_table", 14)):
        m = re.search(rf"^int {name}\((.*?)\);", src, flags=re.M | re.S)
        assert m, f"{name} is not declared in include/macaw_hip.h"
        assert len(m.group(1).split(",")) == len(L.SIGNATURES[name]) == n
        assert name in inspect.getsource(getattr(ops, name[3:]))
    assert int(re.search(r"#define MK_ABI_VERSION (\d+)", src).group(1)) == L.ABI_VERSION
    for phrase in ("Per-row sampling table", "the record's stream where rule 4 has the row index",
                   "it does not depend on where the row sits in the batch", "is greedy: the kernel neither refuses nor loops",
                   "uniform over the workgroup", "not copies of them"):
        assert phrase in src, phrase
    assert src.index("int mk_sample_keep_rows(") < src.index("int mk_sample_rows_table(") < src.index("int mk_logits_process(")
    kernel = open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "sample.hip")).read()
    assert "asm" not in kernel                                            # plain loads and stores, the one arrival atomic
    assert kernel.count("__hip_atomic_fetch_add(state + 2") == 1          # the bookkeeping exists once, shared by the emits


def test_the_library_exports_them_and_bad_arguments_return_codes():
    from macaw_llm_amd import build
    build.build()
    lib = L.load()
    fake = 4096                                                           # never dereferenced: every call below is refused

    def rows(logits=fake, ld=8, n=1, V=8, table=fake, out=fake, dtype=L.MK_BF16):
        return lib.mk_sample_rows_table(logits, ld, n, V, table, 0, out, dtype, None)

    def emit(logits=fake, ld=8, V=8, B=1, tok=fake, done=fake, out=fake, state=fake, table=fake, dtype=L.MK_BF16):
        return lib.mk_decode_emit_sample_table(logits, ld, V, B, 0, 2, tok, done, out, 4, state, table, dtype, None)

    for f in (rows, emit):
        assert f(logits=None) == -1 and f(out=None) == -1 and f(table=None) == -1
        assert f(V=0) == -1 and f(V=-3) == -1 and f(ld=7) == -1
        assert f(V=(1 << 23) + 1, ld=(1 << 23) + 1) == -2                 # MK_ERR_UNSUPPORTED, after the argument checks
        assert f(table=fake + 8) == -2 and f(dtype=7) == -2 and f(dtype=L.MK_FP8) == -2
    assert rows(n=0) == -1 and emit(B=0) == -1 and emit(B=-2) == -1
    assert emit(tok=None) == -1 and emit(done=None) == -1 and emit(state=None) == -1


# ------------------------------------------------------------------------------------------------ 5. resources --
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf"))


@pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                    reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf")
def test_the_table_kernels_use_no_scratch_and_spill_nothing():
    """read from the built library's own metadata: the table kernels hold sample_row<T, false>, sample_row<T, true> and
    the greedy reduction behind one uniform branch, so their registers are the largest form's, with no stack"""
    from macaw_llm_amd import build
    build.build()
    ks = kr.kernels()
    print()
    for stem, twin in (("sample_rows_table_kernel", "sample_rows_kernel"),
                       ("decode_emit_sample_table_kernel", "decode_emit_sample_kernel")):
        mine = {k: v for k, v in ks.items() if stem + "<" in k or f"{stem}I" in k}
        theirs = {k: v for k, v in ks.items() if (twin + "<" in k or f"{twin}I" in k) and k not in mine}
        assert len(mine) == 3 and len(theirs) == 6, (sorted(mine), sorted(theirs))     # bf16, fp16, fp32 (x WARP)
        for k, v in sorted(mine.items()):
            print(f"{v['vgpr_count']:4d} VGPRs  {k[:110]}")
            assert v.get("private_segment_fixed_size", 0) == 0, (k, v)
            assert v.get("vgpr_spill_count", 0) == 0 and v.get("sgpr_spill_count", 0) == 0, (k, v)
            assert v["max_flat_workgroup_size"] == 1024 and v["vgpr_count"] <= 128, (k, v)    # 16 waves of a CU: 512 / 4
        for k, v in sorted(theirs.items()):                               # next to them: the scalar forms they hold
            print(f"{v['vgpr_count']:4d} VGPRs  {k[:110]}")
