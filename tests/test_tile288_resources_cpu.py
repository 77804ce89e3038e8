"""Register budget of gemm_v9's 288 x 256 tile kernel (gemm_*_tile288_kernel), read from the built library as
tests/test_kernel_resources_cpu.py does for the others: 288 accumulators per lane = a[0:255] + 32 VGPRs, the asm block's
v[0:156], no spill, no scratch, one wave per SIMD -- and no compiler-emitted instruction touches an AGPR while the
accumulators live there across asm statements."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
import kernel_resources as kr  # noqa: E402

LLVM_TOOLS = all(os.path.exists(os.path.join(kr.LLVM, t)) for t in ("llvm-objcopy", "llvm-readelf", "llvm-objdump"))
pytestmark = pytest.mark.skipif(not (LLVM_TOOLS and os.path.exists(kr.LIB)),
                                reason="needs the built library and ROCm's llvm-objcopy / llvm-readelf / llvm-objdump")


@pytest.fixture(scope="module")
def built():
    from macaw_llm_amd import build
    build.build()                       # no-op when the stamp matches the sources


def test_the_288_tile_fits_the_register_file_without_spills_or_scratch(built):
    found = {k: v for k, v in kr.kernels().items() if "_tile288_kernel" in k}
    assert len(found) == 2                                  # bf16, f16
    for k, v in found.items():
        assert v.get("agpr_count", 256) == 256, (k, v)
        assert 256 + 157 + 32 <= v["vgpr_count"] <= 512, (k, v)     # (the note counts VGPRs + AGPRs of the unified file)
        assert v.get("vgpr_spill_count", 0) == 0 and v.get("private_segment_fixed_size", 0) == 0, (k, v)
        assert v["max_flat_workgroup_size"] == 256, (k, v)


def test_no_compiler_code_touches_the_288_tiles_accumulator_registers(built):
    """as for *_v9_kernel: the only instructions with an AGPR operand are the MFMAs, the loops' zeroing (2 loop forms x 256)
    and the epilogues' reads (2 forms x 256, every register read equally often)"""
    dis = kr.disassemble("tile288_kernel")
    assert len(dis) == 2
    for sym, lines in dis.items():
        ops, reads = kr.agpr_uses(sym, lines, ("v_mfma_f32_16x16x32_",))
        assert ops["v_accvgpr_write_b32"] == 512 and ops["v_accvgpr_read_b32"] == 512, (sym, dict(ops))
        assert sorted(reads) == list(range(256)) and set(reads.values()) == {2}, sym
        # 144 MFMAs per K-tile in each of the three bodies (steady state, penultimate, last) of both loop forms
        assert sum(i.startswith("v_mfma_f32_16x16x32_") for i in lines) == 2 * 3 * 144, sym
