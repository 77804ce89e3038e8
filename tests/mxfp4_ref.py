"""The MXFP4 weight format of include/macaw_hip.h restated with torch on the CPU (OCP Microscaling v1.0, round to nearest):
e2m1 codes, two per byte (element 2 j in the low nibble of byte j), one E8M0 exponent byte per block of 32 along K.
Every product below is a value times a power of two in float32: exact unless the result is below 2^-126, and such a
result is below the first rounding threshold (0.25) whatever became of it.  So nothing here rounds except the one
documented step: the choice of the nearest e2m1 value, ties to the even code.  The functions compute on the device of
their argument (the CPU in the tests of the format; large weights may be prepared where they already are)."""
import torch

VALUES = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], dtype=torch.float32)


def emin(dtype):
    """smallest block exponent: 0.5 * 2^EMIN is the smallest normal number of the token type"""
    return -13 if dtype == torch.float16 else -125


def _pow2(n):
    """2^n for an integer tensor n in [-126, 127], built from the exponent bits (exact on every device)"""
    return ((n.to(torch.int32) + 127) << 23).view(torch.float32)


def _magnitude_codes(a):
    """a >= 0 (already divided by the block scale) -> 0 ... 7: nearest of VALUES, ties to the even code,
    saturated at 6"""
    return ((a > 0.25).to(torch.int32) + (a >= 0.75).to(torch.int32) + (a > 1.25).to(torch.int32)
            + (a >= 1.75).to(torch.int32) + (a > 2.5).to(torch.int32) + (a >= 3.5).to(torch.int32)
            + (a > 5.0).to(torch.int32))


def block_exponents(W, dtype):
    """E [N, K / 32] (int32): clamp(floor(log2(amax)) - 2, EMIN, 125), EMIN for an all-zero block"""
    Wf = W.detach().float()
    N, K = Wf.shape
    amax = Wf.reshape(N, K // 32, 32).abs().amax(2)
    _, ex = torch.frexp(amax)                                   # amax = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    E = torch.where(amax > 0, ex.to(torch.int32) - 3, torch.full_like(ex, emin(dtype), dtype=torch.int32))
    return E.clamp(emin(dtype), 125)


def _codes(W, E):
    Wf = W.detach().float()
    N, K = Wf.shape
    blk = Wf.reshape(N, K // 32, 32)
    code = _magnitude_codes(blk.abs() * _pow2(-E)[:, :, None])
    code = code | (((blk < 0) & (code != 0)).to(torch.int32) << 3)          # a zero carries no sign
    return code.reshape(N, K)


def _pack(code):
    return (code[:, 0::2] | (code[:, 1::2] << 4)).to(torch.uint8).contiguous()


def quantize(W, dtype):
    """W [N, K], K % 32 == 0 -> (q uint8 [N, K / 2], e uint8 [N, K / 32])"""
    E = block_exponents(W, dtype)
    return _pack(_codes(W, E)), (E + 127).to(torch.uint8)


def unpack(q):
    """q uint8 [N, K / 2] -> codes int32 [N, K], k ascending"""
    q = q.to(torch.int32)
    return torch.stack((q & 15, q >> 4), dim=2).reshape(q.shape[0], -1)


def dequant(q, e):
    """(q, e) -> f32 [N, K]: code value x 2^(e - 127)"""
    code = unpack(q)
    N, K = code.shape
    val = VALUES.to(code.device)[(code & 7).long()] * torch.where((code & 8) != 0, -1.0, 1.0)
    sc = _pow2(e.to(torch.int32) - 127)
    return (val.view(N, K // 32, 32) * sc[:, :, None]).view(N, K)


def snap(W, dtype):
    """W [N, K] -> (values f32, q, e): every block becomes code x power of two with one element planted at +-6 x 2^E at
    the block's arg-max, so that the block maximum re-quantises to the same exponent and quantize(values) reproduces
    q and e exactly (the analogue of test_decode_fp8_gpu._snap_fp8_exact)"""
    Wf = W.detach().float()
    N, K = Wf.shape
    E = block_exponents(Wf, dtype)
    code = _codes(Wf, E).view(N, K // 32, 32)
    blk = Wf.reshape(N, K // 32, 32)
    j = blk.abs().argmax(2, keepdim=True)
    top = torch.where(blk.gather(2, j) < 0, 15, 7).to(torch.int32)
    q = _pack(code.scatter(2, j, top).view(N, K))
    e = (E + 127).to(torch.uint8)
    return dequant(q, e), q, e
