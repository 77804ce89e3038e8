"""CPU checks of the fp8 weight-only decode feature (no kernel is launched): mk_decode_linear_fp8 is declared in the
public header, bound through ctypes with the same number of arguments and exported by the library cross-compiled
for gfx950; generate() and MM_LLMs expose the mode; the engine refuses the fp8 copies outside the decode step."""
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "macaw_hip.h")


def _declared_args(name):
    src = open(HEADER).read()
    m = re.search(r"^int %s\((.*?)\);" % name, src, flags=re.M | re.S)
    assert m, f"{name} is not declared in include/macaw_hip.h"
    return [a.strip() for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_mk_decode_linear_fp8_is_declared_bound_and_exported():
    from macaw_llm_amd import build, lib as L
    args = _declared_args("mk_decode_linear_fp8")
    assert "mk_decode_linear_fp8" in L.SIGNATURES
    assert len(L.SIGNATURES["mk_decode_linear_fp8"]) == len(args) == len(_declared_args("mk_decode_linear")) + 1
    build.build()
    lib = L.load()
    assert hasattr(lib, "mk_decode_linear_fp8")


def test_entry_point_validates_before_it_launches():
    """null pointers / bad prologue -> MK_ERR_BAD_ARG; the domain -> MK_ERR_UNSUPPORTED: decided on the host"""
    from macaw_llm_amd import build, lib as L
    build.build()
    lib = L.load()
    f = lib.mk_decode_linear_fp8
    # (x, Wq, scale, y are fake 16-byte aligned addresses: every call returns before anything is launched)
    assert f(None, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 0, None, 0.0, 1, None) == -1
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 3, None, 0.0, 1, None) == -1
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 1, None, 0.0, 1, None) == -1     # RMSNorm without a weight
    assert f(258, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 0, None, 0.0, 1, None) == -2     # x misaligned
    assert f(256, 256, 513, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 0, None, 0.0, 1, None) == -2     # Wq misaligned
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 96, 0, None, 0.0, 1, None) == -2      # K % 64
    assert f(256, 256, 512, 264, 1024, 2048, 64, None, 0, 1, 64, 256, 0, None, 0.0, 1, None) == -2     # pitch % 16
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 33, 64, 256, 0, None, 0.0, 1, None) == -2    # M > 32
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 17, 64, 256, 1, 4096, 0.0, 1, None) == -2    # prologue: M <= 16
    assert f(256, 4096, 512, 4096, 1024, 2048, 64, None, 0, 8, 64, 4096, 1, 4096, 0.0, 1, None) == -2  # LDS budget
    assert f(256, 256, 512, 256, 1024, 2048, 64, None, 0, 1, 64, 256, 0, None, 0.0, 0, None) == -2     # f32 tokens


def test_generate_and_mm_llms_expose_decode_weights():
    from macaw_llm_amd import modeling as M
    p = inspect.signature(M.LlamaForCausalLM.generate).parameters
    assert "decode_weights" in p and p["decode_weights"].default is None
    assert M.DECODE_WEIGHTS[0] is None
    try:
        M.MM_LLMs.set_decode_weights("fp8")
        assert M.DECODE_WEIGHTS[0] == "fp8"
        with pytest.raises(ValueError):
            M.MM_LLMs.set_decode_weights("int4")
        assert M.DECODE_WEIGHTS[0] == "fp8"
    finally:
        M.MM_LLMs.set_decode_weights(None)
    assert M.DECODE_WEIGHTS[0] is None


def test_ops_and_engine_take_the_fp8_copies():
    from macaw_llm_amd import engine, ops
    assert "w8" in inspect.signature(engine.llama_layer_cached).parameters
    assert inspect.signature(engine.llama_layer_cached).parameters["w8"].default is None
    assert list(inspect.signature(ops.decode_linear_fp8).parameters) == ["x", "Wq", "s", "prologue", "norm_w", "eps",
                                                                        "residual", "out"]
    x = torch.empty((4, 4096), dtype=torch.bfloat16)
    Wq = torch.empty((64, 4096), dtype=torch.uint8)
    assert ops.decode_linear_fp8_ok(x, Wq) and ops.decode_linear_fp8_ok(x, Wq, 1)
    assert not ops.decode_linear_fp8_ok(torch.empty((8, 4096), dtype=torch.bfloat16), Wq, 1)     # 40 KiB of LDS
    assert ops.decode_linear_fp8_ok(torch.empty((32, 4096), dtype=torch.bfloat16), Wq)
    assert not ops.decode_linear_fp8_ok(torch.empty((33, 4096), dtype=torch.bfloat16), Wq)
    assert not ops.decode_linear_fp8_ok(x.float(), Wq)
    assert not ops.decode_linear_fp8_ok(x[:, :96], Wq[:, :96].contiguous())
    with pytest.raises(ValueError, match="w8"):                  # the copies are for the device-position decode step only
        engine.llama_layer_cached(x, 4, 1, 0, None, 8, None, None, None, 32, 1e-6, *([None] * 9), wqkv=None, wgu=None,
                                  t_dev=None, w8=(None,) * 4)
