"""The reference, bounds and tables that tests/test_adamw_edges_gpu.py holds the AdamW kernels of csrc/softmax.hip to
(tests/adamw_ref.py) are themselves checked here, on the CPU:
  - step64 is torch.optim.AdamW in float64 over 5 steps of every hyper case (gradients scaled by grad_scale beforehand);
  - the kernel's statements evaluated in numpy float32 WITHOUT contraction (step32) stay inside E_m, E_v and E_w on every
    element of every hyper case and element type: a correct fp32 kernel passes, the bounds need nothing from a GPU;
  - each of the seven wrong variants leaves E_w or E_v on some hyper case, i.e. the bounds would catch that bug;
  - the size and list tables reach every loop of both kernels and both outcomes of the multi kernel's `two` test
    (branch_census);
  - the host's fp32 bias corrections (mk_adamw_bias_correction, the library loaded without a GPU) are within the 2 u the
    bound grants them, and step < 1 is refused."""
import ctypes

import numpy as np
import pytest
import torch

import adamw_ref as R

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
N = 2048 + 3


@pytest.mark.parametrize("case", list(R.HYPER_CASES))
def test_step64_is_torch_adamw_in_float64(case):
    h = R.HYPER_CASES[case]
    w, m, v, _ = R.make_state(case, N, torch.float32)
    p = torch.nn.Parameter(w.double().clone())
    opt = torch.optim.AdamW([p], lr=h.lr, betas=(h.b1, h.b2), eps=h.eps, weight_decay=h.wd, foreach=False)
    opt.state[p] = {"step": torch.tensor(float(h.step - 1)), "exp_avg": m.double().clone(),
                    "exp_avg_sq": v.double().clone()}
    cur = (w.double(), m.double(), v.double())
    gen = torch.Generator().manual_seed(5)
    for k in range(5):
        g = torch.randn(N, generator=gen, dtype=torch.float64) * h.sigma_g
        g[R.zero_run(N)] = 0
        p.grad = g * h.gs
        opt.step()
        s = R.step64(*cur, g, h.lr, h.b1, h.b2, h.eps, h.wd, h.step + k, h.gs)
        cur = (s.w, s.m, s.v)
        st = opt.state[p]
        for name, got, want in (("w", s.w, p.detach()), ("m", s.m, st["exp_avg"]), ("v", s.v, st["exp_avg_sq"])):
            # 1e-12 relative; an element that happens to sit at zero is held to 1e-12 of the tensor's typical size
            atol = 1e-12 * float(want.abs().median())
            torch.testing.assert_close(got, want, rtol=1e-12, atol=atol, msg=lambda s_: f"{case} step {k} {name}: {s_}")
    z = R.zero_run(N)
    assert z.stop - z.start == 37 and not cur[1][z].any() and not cur[2][z].any()
    assert all(torch.isfinite(t).all() for t in cur)


@pytest.mark.parametrize("bug", [None, *R.BUGS])
def test_flagged_restatement_without_a_bug_is_step64(bug):
    """the mutants are built from one flagged restatement: with no flag it is step64 bit for bit, with a flag it is not"""
    same = True
    for case, h in R.HYPER_CASES.items():
        w, m, v, g = R.make_state(case, N, torch.bfloat16)
        s = R.step64(w, m, v, g, *R.hyper_args(h))
        got = R._flagged(bug)(w, m, v, g, *R.hyper_args(h))
        same = same and all(torch.equal(a, b) for a, b in zip(got, (s.w, s.m, s.v)))
    assert same == (bug is None)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", list(R.HYPER_CASES))
def test_fp32_evaluation_in_kernel_order_is_inside_the_bounds(case, dtype):
    h = R.HYPER_CASES[case]
    w, m, v, g = R.make_state(case, 40000, dtype)
    s = R.step64(w, m, v, g, *R.hyper_args(h))
    w32, m32, v32 = R.step32(w, m, v, g, *R.hyper_args(h))
    rm = R.assert_within(torch.from_numpy(m32), s.m, s.E_m, f"{case} m")
    rv = R.assert_within(torch.from_numpy(v32), s.v, s.E_v, f"{case} v")
    rw = R.assert_within(torch.from_numpy(w32), s.w, s.E_w, f"{case} w")
    print(f"{case} {dtype}: worst err / bound  m {rm:.3f}  v {rv:.3f}  w {rw:.3f}")
    z = R.zero_run(40000)
    assert z.stop - z.start == 37
    assert not s.m[z].any() and not s.v[z].any() and not m32[z].any() and not v32[z].any()
    lr, wd = h.lr, h.wd
    assert torch.equal(s.w[z], w[z].double() - lr * wd * w[z].double())


def test_bounds_resolve_the_update():
    """the bound is a statement about the UPDATE, not about the weight: with w ~ 0.02 the term u |w| (1e-9) is small even
    against a 3e-5 step, so on the typical element of every case E_w is below a thousandth of |w' - w|"""
    for case, h in R.HYPER_CASES.items():
        w, m, v, g = R.make_state(case, 40000, torch.bfloat16)
        s = R.step64(w, m, v, g, *R.hyper_args(h))
        ratio = float((s.E_w / (s.w - w.double()).abs().clamp_min(1e-300)).median())
        assert ratio < 1e-3, (case, ratio)


@pytest.mark.parametrize("bug", R.BUGS)
def test_every_mutant_leaves_the_bounds(bug):
    """each wrong variant is outside E_w or E_v on most elements of at least one hyper case (and the table printed with
    -s shows where); none had to be dropped"""
    caught = {}
    for case, h in R.HYPER_CASES.items():
        n = 4096
        w, m, v, g = R.make_state(case, n, torch.bfloat16)
        s = R.step64(w, m, v, g, *R.hyper_args(h))
        w2, m2, v2 = R.mutants[bug](w, m, v, g, *R.hyper_args(h))
        live = n - 37
        caught[case] = (R.exceeds(w2, s.w, s.E_w) / live, R.exceeds(v2, s.v, s.E_v) / live)
    print(bug, {k: f"w {a:.2f} v {b:.2f}" for k, (a, b) in caught.items()})
    assert max(max(a, b) for a, b in caught.values()) > 0.9, caught


def test_mutants_are_the_listed_ones():
    assert set(R.mutants) == {"eps_inside_sqrt", "gs_missing_from_v", "bc1_for_both", "bc_at_previous_step",
                              "l2_instead_of_decoupled", "decay_after_update", "update_from_old_m"}


def _chunk():
    from macaw_llm_amd import lib as L
    return int(L.load().mk_adamw_chunk())


def test_single_sizes_reach_every_loop():
    cen = {(n, cap): R.branch_census(n, max_blocks=cap) for n, cap in R.SIZES_SINGLE}
    for (n, cap), c in cen.items():
        assert c["n_vector"] + c["n_tail"] == n and len(c["tail"]) == n
        assert int(c["tail"].sum()) == c["n_tail"] == n % 4
    assert any(c["n_vector"] == 0 and c["n_tail"] > 0 for c in cen.values()), "tail only"
    assert any(c["n_vector"] > 0 and c["n_tail"] == 0 for c in cen.values()), "vector only"
    assert any(c["n_vector"] > 0 and c["n_tail"] == 3 for c in cen.values()), "vector and the longest tail"
    assert cen[(2048, 0)]["blocks"] == 1 and cen[(2048, 0)]["thread_trips"] == {2}
    assert cen[(2051, 0)]["blocks"] == 1 and cen[(2051, 0)]["n_tail"] == 3
    assert cen[(10242, 0)]["blocks"] == 5 and cen[(10242, 0)]["thread_trips"] == {2} and cen[(10242, 0)]["n_tail"] == 2
    big = cen[(5 * 2 ** 20 + 3, 0)]
    assert big["blocks"] == R.SINGLE_MAX_BLOCKS and big["thread_trips"] == {2, 3} and big["n_tail"] == 3
    assert (5 * 2 ** 20 + 3) // 8 // 256 > R.SINGLE_MAX_BLOCKS, "the cap really binds"
    capped = cen[(4099, 1)]
    assert capped["blocks"] == 1 and capped["thread_trips"] == {4} and capped["n_tail"] == 3
    assert R.branch_census(4099)["blocks"] > 1, "without the cap it would be more than one block"
    assert cen[(4, 0)]["thread_trips"] == {0, 1} and cen[(7, 0)]["thread_trips"] == {0, 1}


def test_multi_sizes_and_lists_reach_every_loop_and_both_two_outcomes():
    C = _chunk()
    sizes = R.SIZES_MULTI(C)
    assert len(sizes) == 15 and len(set(sizes)) == 15 and min(sizes) == 1
    cen = {n: R.branch_census(n, chunk=C) for n in sizes}
    for n, c in cen.items():
        assert c["n_vector"] + c["n_tail"] == n and c["blocks"] == (n + C - 1) // C
    assert cen[1]["n_vector"] == 0 and cen[3]["n_vector"] == 0 and cen[3]["two"] == set()
    assert cen[4]["two"] == {False} and cen[1020]["two"] == {False} and cen[1024]["two"] == {False}
    assert cen[1024]["thread_trips"] == {1} and cen[1020]["thread_trips"] == {0, 1}
    assert cen[1028]["two"] == {True, False} and cen[1028]["n_tail"] == 0
    c = cen[1031]
    assert c["two"] == {True, False} and c["n_tail"] == 3 and int((c["group"] == 1).sum()) == 4, "group 1: thread 0 only"
    assert cen[2048]["two"] == {True} and cen[2048]["thread_trips"] == {1}
    assert cen[2052]["two"] == {True, False} and cen[2052]["thread_trips"] == {1, 2}
    assert cen[3079]["n_tail"] == 3 and int(cen[3079]["trip"].max()) == 1 and cen[3079]["two"] == {True, False}
    assert cen[C]["blocks"] == 1 and cen[C]["two"] == {True} and cen[C]["n_tail"] == 0
    assert cen[C - 1]["blocks"] == 1 and cen[C - 1]["n_tail"] == 3
    assert cen[C + 1]["blocks"] == 2 and cen[C + 1]["n_tail"] == 1, "a last slice of one element"
    assert cen[C + 1031]["blocks"] == 2 and cen[C + 1031]["two"] == {True, False}
    assert cen[3 * C - 4]["blocks"] == 3 and cen[3 * C - 4]["n_tail"] == 0 and cen[3 * C - 4]["two"] == {True, False}
    for k in (0, 1):
        assert any(((c["group"] == k) & (c["trip"] > 0)).any() for c in cen.values()), f"group {k} beyond the first trip"
    lists = R.LISTS(C)
    assert [len(v) for v in lists.values()] == [1, 2, 3, 17, 3]
    assert lists["single_element_in_the_middle"][1] == 1 and lists["empty_in_the_middle"][1] == 0
    assert set(lists["seventeen"]) >= set(sizes), "the long list mixes every size of the table"
    starts = R.chunk_starts(lists["empty_in_the_middle"], C)
    assert starts[1] == starts[2] and starts[-1] == 3, "the empty tensor owns no block"
    s17 = R.chunk_starts(lists["seventeen"], C)
    assert s17[-1] == sum((n + C - 1) // C for n in lists["seventeen"]) and s17[-1] > 17


@pytest.mark.parametrize("beta", [0.9, 0.95, 0.98, 0.999])
def test_host_bias_correction_is_within_two_u(beta):
    from macaw_llm_amd import lib as L
    lib = L.load()
    out = (ctypes.c_float * 2)()
    other = 0.999 if beta != 0.999 else 0.9
    for step in (1, 2, 3, 7, 10, 100, 1000, 5000, 200000):
        assert lib.mk_adamw_bias_correction(beta, other, step, out) == 0
        want = 1.0 - R.f32(beta) ** step
        want_o = 1.0 - R.f32(other) ** step
        assert R.bias_corrections64(beta, other, step) == (want, want_o)
        assert abs(float(out[0]) - want) <= 2 * R.U, (beta, step, float(out[0]), want)
        assert abs(float(out[1]) - want_o) <= 2 * R.U, (other, step, float(out[1]), want_o)
        # numpy's powf, which step32 uses, is held to the same
        assert abs(float(np.float32(1) - np.power(np.float32(beta), np.float32(step), dtype=np.float32)) - want) <= 2 * R.U
        if step == 200000:
            assert float(out[0]) == 1.0 and float(out[1]) == 1.0 and want == 1.0
    for step in (0, -1):
        assert lib.mk_adamw_bias_correction(beta, other, step, out) != 0
    assert lib.mk_adamw_bias_correction(beta, other, 1, None) != 0
