"""CPU checks of the MXFP4 weight-only decode feature (no kernel is launched): mk_mxfp4_quantize_rows and
mk_decode_linear_mxfp4 are declared in the public header, bound through ctypes with the same number of arguments and
exported by the library cross-compiled for gfx950; the entry point decides its domain on the host; generate() and
MM_LLMs expose the mode; the format's restatement (tests/mxfp4_ref.py) rounds and saturates as OCP MX v1.0 says; the new
kernels stay inside the register budget of the streaming kernels."""
import inspect
import os
import re
import sys

import pytest
import torch

import mxfp4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import kernel_resources as kr  # noqa: E402

LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf"))


def _declared_args(name):
    src = open(HEADER).read()
    m = re.search(r"^int %s\((.*?)\);" % name, src, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/macaw_hip.h"
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_both_symbols_are_declared_bound_and_exported():
    from macaw_llm_amd import build, lib as L
    build.build()
    lib = L.load()
    for name, n in (("mk_mxfp4_quantize_rows", 10), ("mk_decode_linear_mxfp4", 18)):
        args = _declared_args(name)
        assert name in L.SIGNATURES
        assert len(L.SIGNATURES[name]) == len(args) == n
        assert hasattr(lib, name)
    # (the e4m3 entry point with the scale pointer replaced by exponent pointer + pitch)
    assert len(_declared_args("mk_decode_linear_mxfp4")) == len(_declared_args("mk_decode_linear_fp8")) + 1
    assert "decode_mxfp4.hip" in build.SOURCES


def test_entry_point_validates_before_it_launches():
    """null pointers / bad prologue -> MK_ERR_BAD_ARG; the domain -> MK_ERR_UNSUPPORTED: decided on the host"""
    from macaw_llm_amd import build, lib as L
    build.build()
    f = L.load().mk_decode_linear_mxfp4

    # x, Wq, e, y are fake aligned addresses: every call returns before anything is launched
    def call(x=256, ldx=256, Wq=512, ldw=128, e=1024, lde=8, y=2048, ldy=64, M=1, N=64, K=256, pro=0, nw=None, dtype=1):
        return f(x, ldx, Wq, ldw, e, lde, y, ldy, None, 0, M, N, K, pro, nw, 0.0, dtype, None)

    assert call(x=None) == -1 and call(Wq=None) == -1 and call(e=None) == -1 and call(y=None) == -1
    assert call(pro=3) == -1
    assert call(pro=1) == -1                                    # RMSNorm without a weight
    assert call(x=258) == -2 and call(Wq=513) == -2             # x / Wq off a 16-byte boundary
    assert call(e=1026) == -2                                   # e off a 4-byte boundary
    assert call(K=192, ldx=192, ldw=96, lde=8) == -2            # K % 128
    assert call(ldw=136) == -2 and call(ldw=112) == -2          # ldw % 16, ldw < K / 2
    assert call(lde=10) == -2 and call(lde=4) == -2             # lde % 4, lde < K / 32
    assert call(M=33) == -2                                     # plain: M <= 32
    assert call(M=17, pro=1, nw=4096) == -2                     # prologue: M <= 16
    assert call(M=17, pro=2, ldx=512) == -2
    assert call(M=8, K=4096, ldx=4096, ldw=2048, lde=128, pro=1, nw=4096) == -2     # LDS budget
    assert call(dtype=0) == -2                                  # f32 tokens
    q = L.load().mk_mxfp4_quantize_rows
    assert q(None, 4, 128, 128, 1, 512, 64, 1024, 4, None) == -1
    assert q(256, 4, 128, 128, 0, 512, 64, 1024, 4, None) == -2         # f32 input
    assert q(256, 4, 144, 144, 1, 512, 80, 1024, 5, None) == -2         # cols % 32
    assert q(258, 4, 128, 128, 1, 512, 64, 1024, 4, None) == -2         # x misaligned
    assert q(256, 4, 128, 128, 1, 512, 72, 1024, 4, None) == -2         # ldq % 16


def test_generate_and_mm_llms_expose_the_mxfp4_mode():
    from macaw_llm_amd import modeling as M
    p = inspect.signature(M.LlamaForCausalLM.generate).parameters
    assert "decode_weights" in p and p["decode_weights"].default is None
    assert "mxfp4" in M.LlamaForCausalLM.generate.__doc__
    assert M.DECODE_WEIGHTS[0] is None
    try:
        M.MM_LLMs.set_decode_weights("mxfp4")
        assert M.DECODE_WEIGHTS[0] == "mxfp4"
        with pytest.raises(ValueError):
            M.MM_LLMs.set_decode_weights("int4")
        assert M.DECODE_WEIGHTS[0] == "mxfp4"                   # a refused value leaves the state untouched
    finally:
        M.MM_LLMs.set_decode_weights(None)
    assert M.DECODE_WEIGHTS[0] is None


def test_decode_linear_mxfp4_ok_truth_table():
    from macaw_llm_amd import ops
    assert list(inspect.signature(ops.decode_linear_mxfp4).parameters) == ["x", "Wq", "e", "prologue", "norm_w", "eps",
                                                                          "residual", "out"]
    bf = torch.bfloat16
    x = lambda M, K, dtype=bf: torch.empty((M, K), dtype=dtype)  # noqa: E731
    codes = lambda K: torch.empty((64, K // 2), dtype=torch.uint8)  # noqa: E731
    master = lambda K: torch.empty((64, K), dtype=bf)  # noqa: E731
    for W in (codes, master):                                   # the codes, or the 16-bit weight they will be made from
        assert ops.decode_linear_mxfp4_ok(x(4, 4096), W(4096)) and ops.decode_linear_mxfp4_ok(x(4, 4096), W(4096), 1)
        assert ops.decode_linear_mxfp4_ok(x(4, 4096), W(4096), 2)
        assert ops.decode_linear_mxfp4_ok(x(8, 4096), W(4096)) and not ops.decode_linear_mxfp4_ok(x(8, 4096), W(4096), 1)
        assert not ops.decode_linear_mxfp4_ok(x(8, 4096), W(4096), 2)                   # 40 KiB of LDS
        assert ops.decode_linear_mxfp4_ok(x(32, 4096), W(4096)) and not ops.decode_linear_mxfp4_ok(x(33, 4096), W(4096))
        assert not ops.decode_linear_mxfp4_ok(x(32, 4096), W(4096), 1)                  # prologue: M <= 16
        for M in (4, 8, 32, 33):
            assert not ops.decode_linear_mxfp4_ok(x(M, 192), W(192))                    # K % 128 (the 16-bit and e4m3 kernels take it)
            assert not ops.decode_linear_mxfp4_ok(x(M, 704), W(704))
        assert ops.decode_linear_ok(x(4, 704), master(704)) and ops.decode_linear_ok(x(4, 192), master(192))
        assert not ops.decode_linear_mxfp4_ok(x(4, 4096, torch.float32), W(4096))
        assert ops.decode_linear_mxfp4_ok(x(4, 4096, torch.float16), W(4096))
        assert not ops.decode_linear_mxfp4_ok(x(4, 4096), W(8192)[:, ::2])              # not contiguous


# ------------------------------------------------------------------------------------------------ the format --
def _block(vals, fill=0.0):
    b = torch.full((1, 32), fill)
    b[0, :len(vals)] = torch.tensor(vals)
    return b


def test_ref_rounds_ties_to_the_even_code():
    """a block whose amax is 4 has E = 0: its elements are rounded as they stand"""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    for sgn in (1.0, -1.0):
        q, e = R.quantize(_block([4.0] + [sgn * t for t in ties]), torch.bfloat16)
        assert int(e[0, 0]) == 127
        got = R.dequant(q, e)[0, 1:8]
        assert got.tolist() == [sgn * v if v else 0.0 for v in (0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0)], got
    c = R.unpack(R.quantize(_block([4.0, -0.25, -0.2]), torch.bfloat16)[0])
    assert c[0, 1] == 0 and c[0, 2] == 0                        # a zero code carries no sign
    # just off the ties
    q, e = R.quantize(_block([4.0, 0.2500001, 0.7499999, 1.2500001, 1.7499999, 2.5000002, 3.4999998, 5.000001]), torch.bfloat16)
    assert R.dequant(q, e)[0, 1:8].tolist() == [0.5, 0.5, 1.5, 1.5, 3.0, 3.0, 6.0]


def test_ref_saturates_picks_the_block_exponent_and_clamps_it_per_dtype():
    for E in (-20, 0, 9):
        s = 2.0 ** E
        q, e = R.quantize(_block([7.9 * s, -7.9 * s, 6.9 * s, 4.0 * s, 0.5 * s]), torch.bfloat16)
        assert int(e[0, 0]) == E + 127                          # floor(log2(7.9)) - 2 = 0
        assert R.dequant(q, e)[0, :5].tolist() == [6.0 * s, -6.0 * s, 6.0 * s, 4.0 * s, 0.5 * s]
    assert R.emin(torch.bfloat16) == -125 and R.emin(torch.float16) == -13
    for dtype in (torch.bfloat16, torch.float16):
        q, e = R.quantize(torch.zeros(2, 64), dtype)            # all-zero blocks: E = EMIN, codes 0
        assert (e == R.emin(dtype) + 127).all() and (q == 0).all()
        assert (R.dequant(q, e) == 0).all()
        tiny = 2.0 ** (R.emin(dtype) - 4)                       # amax below 4 * 2^EMIN: the exponent is clamped
        q, e = R.quantize(_block([8 * tiny, 16 * tiny, tiny]), dtype)
        assert int(e[0, 0]) == R.emin(dtype) + 127
        d = R.dequant(q, e)[0, :3]
        assert d.tolist() == [0.5 * 2.0 ** R.emin(dtype), 2.0 ** R.emin(dtype), 0.0]
        # ... and every non-zero de-quantised value is a normal number of the type
        assert float(d[0]) == torch.finfo(dtype).smallest_normal
    q, e = R.quantize(_block([3.0e38]), torch.bfloat16)         # floor(log2) = 127: clamped at 125, saturated
    assert int(e[0, 0]) == 252 and R.dequant(q, e)[0, 0] == 6.0 * 2.0 ** 125


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_ref_quantize_reproduces_snapped_weights(dtype):
    g = torch.Generator().manual_seed(5)
    W = torch.randn(24, 256, generator=g) * 0.05
    W[3, 32:64] = 0                                             # an all-zero block gets a planted 6 x 2^EMIN
    W[5] *= 1e-3
    val, q, e = R.snap(W, dtype)
    assert torch.equal(val.to(dtype).float(), val)              # exact in the token type
    q2, e2 = R.quantize(val, dtype)
    assert torch.equal(q2, q) and torch.equal(e2, e)
    assert torch.equal(R.dequant(q2, e2), val)
    code = R.unpack(q).view(24, 8, 32) & 7
    assert ((code == 7).sum(2) >= 1).all()                      # the planted maximum of every block
    # ordinary weights, blocks whose exponent is not clamped: the block is scaled into [4, 8), where the e2m1 grid's
    # widest step is 2 (4 -> 6) and saturation loses less than 2, and every |x - q| <= 0.25 |x| above the first step
    qo, eo = R.quantize(W, torch.bfloat16)
    err = (R.dequant(qo, eo) - W).view(24, 8, 32).abs().amax(2)
    amax = W.view(24, 8, 32).abs().amax(2)
    assert (err <= 0.25 * amax).all()


# --------------------------------------------------------------------------------------------- kernel resources --
@pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                    reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf")
def test_the_mxfp4_kernels_keep_the_streaming_kernels_budget():
    """both element types exist; at most 128 VGPRs (two 8-wave workgroups per CU, the bound
    test_kernel_resources_cpu sets for the weight-streaming kernels), no spill, no scratch"""
    from macaw_llm_amd import build
    build.build()
    ks = kr.kernels()
    found = {}
    for ns in ("e_bf16::", "e_f16::"):
        lin = {k: v for k, v in ks.items() if ns in k and "decode_linear_mxfp4_kernel<" in k}
        assert len(lin) == 7, sorted(lin)                       # plain x 3 (8 / 16 waves, two token tiles), 2 prologues x 2
        found.update(lin)
    quant = {k: v for k, v in ks.items() if "mxfp4_quantize_rows_kernel" in k}
    assert len(quant) == 2, sorted(quant)                       # one per element type
    found.update(quant)
    for k, v in found.items():
        assert v["vgpr_count"] <= 128, (k, v)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (k, v)
