"""Register budget of the grouped-launch kernels (csrc/gemm_v9_impl.inc gemm_*_grp_kernel), read from the built library as
tests/test_kernel_resources_cpu.py does for gemm_v9: the generated K loop owns a[0:255] across asm statements, so the kernel
must keep all 256 AGPRs, spill nothing, use no scratch, run one wave per SIMD (workgroup size 256) -- and no compiler-made
instruction may touch an AGPR between the loop and the epilogue's reads."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
import kernel_resources as kr  # noqa: E402

LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf", "llvm-objdump"))
pytestmark = pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                                reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf / llvm-objdump")


@pytest.fixture(scope="module")
def ks():
    from macaw_llm_amd import build
    build.build()                       # no-op when the stamp matches the sources
    return {k: v for k, v in kr.kernels().items() if "_grp_kernel<" in k}


def test_main_plus_filler_and_filler_only_exist_for_both_element_types(ks):
    assert sorted(ks) == sorted(f"void e_{t}::gemm_{t}_grp_kernel<{m}>(mkg::GrpArgs)" for t in ("bf16", "f16")
                                for m in ("true", "false")), sorted(ks)
    assert not [k for k in ks if "v9_kernel" in k or "v7_kernel" in k]


def test_256_agprs_no_spill_no_scratch_one_wave_per_simd(ks):
    for k, v in ks.items():
        assert v.get("agpr_count", 256) == 256, (k, v)
        assert 256 + 88 <= v["vgpr_count"] <= 512, (k, v)   # (the note counts VGPRs + AGPRs of the unified file)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)


def test_only_mfmas_zeroing_writes_and_the_epilogue_reads_touch_an_agpr():
    dis = kr.disassemble("grp_kernel")
    assert len(dis) == 4
    for sym, lines in dis.items():
        loops = 4 if "Lb1E" in sym else 2          # <true>: the first / walking loop of both layouts; <false>: of one
        ops, reads = kr.agpr_uses(sym, lines, ("v_mfma_f32_16x16x32_",))
        assert ops["v_accvgpr_write_b32"] == 256 * loops, (sym, dict(ops))
        assert sorted(reads) == list(range(256)) and set(reads.values()) == {1}, sym      # ONE epilogue form
