"""CPU checks of the generated K loop of gemm_v9's 288 x 256 x 64 tile (scripts/gen_v9_loop.py --tile288 ->
macaw_llm_amd/csrc/gemm_v9_loop288.inc; kernel: gemm_bf16_tile288_kernel in gemm_v9_impl.inc):

  * the committed .inc is what the generator writes, and its LDS layout fits the budget;
  * the piece -> LDS address map of the LDS-DMA (C++: v7_voffset, v9_tile_request) against the fragment read addresses
    (C++: v9_read_offset16, the kernel's adA / adB): every lane of every fragment read finds the row and the 16-byte chunk
    the MFMA operand layout wants, and a wave's voffsets are piece 0's plus strides, as the asm derives them;
  * a single-wave SIMULATION of the stream for nk = 2, 3, 4, 5, 16, plain and walking form, every wave: no LDS slot is
    refilled before a barrier that follows its last read, no fragment is read before its pieces were waited for (counted
    vmcnt) and published by a barrier, M0 is written at least two instructions ahead of its load, every piece of every
    K-tile is requested exactly once, every MFMA multiplies the fragments it should, and every accumulator sees the
    K-tiles and k32-steps in ascending order (the 256 tile's order: that is what makes the results the same bits).

No GPU involved: the numerics are covered by tests/test_gemm_tile288_gpu.py."""
import contextlib
import importlib.util
import io
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("gen_v9_loop", os.path.join(ROOT, "scripts", "gen_v9_loop.py"))
gen = importlib.util.module_from_spec(spec)
spec.loader.exec_module(gen)

A_SLOT, B_SLOT, B_BASE, LDS = gen.A_SLOT288, gen.B_SLOT288, gen.B_BASE288, gen.LDS288
NPA, NPB = 9, 8             # pieces per wave and K-tile


def test_committed_inc_is_generated_and_the_other_file_is_untouched():
    for fn, name in ((gen.main288, "gemm_v9_loop288.inc"), (gen.main, "gemm_v9_loop.inc")):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fn("-")
        with open(os.path.join(ROOT, "macaw_llm_amd", "csrc", name)) as f:
            assert f.read() == buf.getvalue(), f"run scripts/gen_v9_loop.py ({name})"


def test_lds_layout_fits_the_budget_and_matches_the_kernel():
    assert A_SLOT == 288 * 64 * 2 and B_SLOT == 256 * 64 * 2 and B_BASE == 2 * A_SLOT
    assert LDS == 139264 <= 163840          # LDS9 of gemm_v9_impl.inc = the CU's 160 KiB
    with open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "gemm_v9_loop288.inc")) as f:
        txt = f.read()
    for name, val in (("V9_LDS288", LDS), ("V9_A_SLOT288", A_SLOT), ("V9_B_BASE288", B_BASE)):
        assert re.search(rf"#define {name} {val}\n", txt)
    with open(os.path.join(ROOT, "macaw_llm_amd", "csrc", "gemm_v9_impl.inc")) as f:
        impl = f.read()
    # the kernel takes the slots from the generated file and places the waves' read bases as this file assumes
    assert "A_SLOT288 = V9_A_SLOT288, B_BASE288 = V9_B_BASE288, LDS288 = V9_LDS288" in impl
    assert "adA = lds0 + wr * (A_SLOT288 / 2) + v9_read_offset16<false>(l)" in impl
    assert "adB = lds0 + B_BASE288 + wc * HALF_BYTES + v9_read_offset16<false>(l)" in impl


# ---- the C++ formulas, restated (gemm_lds_image.inc v7_voffset<false>, gemm_v9_impl.inc v9_read_offset16<false>) ------
def v7_voffset(row0, R, ld, half, p, l):
    r = p * 8 + (l >> 3)
    kc = (l & 7) ^ ((r >> 1) & 7)
    gr = min(row0 + half * 128 + r, R - 1) - row0
    return gr * ld * 2 + kc * 16


def v9_read_offset16(l):
    row = l & 15
    return row * 128 + (((l >> 4) ^ ((row >> 1) & 7)) << 4)


@pytest.mark.parametrize("rows,npw", [(288, NPA), (256, NPB)])
def test_piece_map_against_the_read_offsets(rows, npw):
    """v9_operand_setup: piece w + 4 i of a wave = v7_voffset(half i >> 2, piece w + 4 (i & 3)); v9_tile_request: it lands
    at (w + 4 i) * 1024 + 16 l of the slot.  Build the image (LDS byte -> global row, 16-byte chunk) and read it back as
    the loop does: fragment f of k32-step h of wave half `wh` at  wh * rows / 2 * 128 + (v9_read_offset16(l) ^ (h << 6))
    + 2048 f  must hold row  wh * rows / 2 + 16 f + (l & 15),  chunk 4 h + (l >> 4)  (the A / B operand layout of
    v_mfma_f32_16x16x32: lane l = row l & 15, k = 8 (l >> 4) .. + 7)."""
    ld, row0, R = 4096 + 8, 2 * rows, 8 * rows
    image = {}
    for w in range(4):
        base = [v7_voffset(row0, R, ld, 0, w, l) for l in range(64)]
        for i in range(npw):
            for l in range(64):
                vo = v7_voffset(row0, R, ld, i >> 2, w + 4 * (i & 3), l)
                assert vo == base[l] + i * 32 * ld * 2          # the asm: v_add_u32 of iA / iB = 32 rows, i times
                addr = (w + 4 * i) * 1024 + 16 * l
                assert addr not in image and addr + 16 <= rows * 128
                image[addr] = (vo // (ld * 2), (vo % (ld * 2)) // 16)
    assert len(image) == rows * 8
    for wh in range(2):
        for h in range(2):
            for f in range(rows // 32):
                addrs = []
                for l in range(64):
                    addr = wh * (rows // 2) * 128 + (v9_read_offset16(l) ^ (h << 6)) + 2048 * f
                    assert image[addr] == (wh * (rows // 2) + 16 * f + (l & 15), 4 * h + (l >> 4)), (wh, h, f, l)
                    addrs.append(addr)
                # (ds_read_b128 is served in four groups of 16 lanes: lanes 0-3 + 12-15 + 16-19 + 28-31 ..., each group at
                # the conflict-free rate needs its 16 x 4 banks distinct; the swizzle is the 256 tile's, checked there)


# ---- single-wave simulation ---------------------------------------------------------------------------------------
class Sim:
    def __init__(self, nk, w):
        self.nk, self.w = nk, w
        self.stA, self.stB = 128, 128
        self.s, self.v = {}, {}
        self.m0, self.m0_age = None, 99
        self.scc, self.scc_fresh = None, False
        self.t = 0
        self.barriers = []
        # LDS in groups of 4 KiB = the four waves' pieces 4 i .. 4 i + 3: the other waves run the same stream between the same
        # barriers, so this wave's piece w + 4 i stands for its group
        self.lds = {}            # group index -> dict(op, tile, group (inside the tile), landed)
        self.inflight = set()    # groups with a request outstanding
        self.vmq = []
        self.lgkm = []
        self.regs = {}
        self.last_read = {}
        self.requested = {}
        self.mfma_log = []
        # what v9_tile_request<288> has issued: tile 0 (A and B piece by piece, then A's ninth), then A(1)
        for i in range(8):
            self.dma("A", (w + 4 * i) * 1024, 0, i)
            self.dma("B", B_BASE + (w + 4 * i) * 1024, 0, i)
        self.dma("A", (w + 32) * 1024, 0, 8)
        for i in range(NPA):
            self.dma("A", A_SLOT + (w + 4 * i) * 1024, 1, i)

    def dma(self, op, addr, tile, i):
        assert 0 <= tile < self.nk, ("request of a K-tile that does not exist", op, tile)
        assert (op, tile, i) not in self.requested, ("piece requested twice", op, tile, i)
        self.requested[(op, tile, i)] = self.t
        base, size = (0, A_SLOT) if op == "A" else (B_BASE, B_SLOT)
        assert base <= addr < base + 2 * size and addr % 1024 == 0 and addr + 1024 <= LDS
        slot, off = divmod(addr - base, size)
        assert slot == tile & 1, ("tile T lives in slot T & 1", op, tile, addr)
        assert off == (self.w + 4 * i) * 1024
        k = addr // 4096
        assert k not in self.inflight
        lr = self.last_read.get(k)
        if lr is not None:      # WAR: a barrier lies between the last read of the old content and this request
            assert any(lr < b <= self.t for b in self.barriers), ("refilled before the barrier after its last read", op, tile, i)
        self.inflight.add(k)
        self.vmq.append(dict(op=op, k=k, tile=tile, group=i))

    def val(self, tok):
        tok = tok.strip()
        if re.fullmatch(r"s\d+", tok):
            return self.s[int(tok[1:])]
        if re.fullmatch(r"v\d+", tok):
            return self.v[int(tok[1:])]
        return int(tok, 0)

    def run(self, lines):
        labels = {l[:-1]: n for n, l in enumerate(lines) if l.endswith(":")}
        pc = steps = 0
        while pc < len(lines):
            steps += 1
            assert steps < 200000
            l = lines[pc]
            pc += 1
            self.t += 1
            self.m0_age += 1
            if l.endswith(":") or l.startswith((".p2align", "s_nop", "v_accvgpr_write")):
                continue
            op, _, rest = l.partition(" ")
            a = [x.strip() for x in rest.split(",")] if rest else []
            fresh, self.scc_fresh = self.scc_fresh, False
            if op in ("s_mov_b32", "s_add_u32", "s_sub_u32", "s_xor_b32", "s_lshl_b32", "v_mov_b32", "v_add_u32", "v_xor_b32"):
                if op.endswith("mov_b32"):
                    r = self.val(a[1])
                else:
                    x, y = self.val(a[1]), self.val(a[2])
                    r = {"add": x + y, "sub": x - y, "xor": x ^ y, "lsh": x << y}[op[2:5]]
                r &= 0xffffffff
                if a[0] == "m0":
                    self.m0, self.m0_age = r, 0
                elif a[0][0] == "s":
                    self.s[int(a[0][1:])] = r
                else:
                    self.v[int(a[0][1:])] = r
            elif op in ("s_cmp_eq_u32", "s_cmp_lg_u32"):
                x, y = self.val(a[0]), self.val(a[1])
                self.scc, self.scc_fresh = ((x == y) if op == "s_cmp_eq_u32" else (x != y)), True
            elif op == "s_cbranch_scc1":
                assert fresh, "SCC consumer not adjacent to its s_cmp"
                if self.scc:
                    pc = labels[a[0]]
            elif op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", rest)
                if m:
                    while len(self.vmq) > int(m.group(1)):
                        p = self.vmq.pop(0)
                        self.inflight.discard(p["k"])
                        self.lds[p["k"]] = dict(op=p["op"], tile=p["tile"], group=p["group"], landed=self.t)
                if "lgkmcnt(0)" in rest:
                    for r0, tag in self.lgkm:
                        self.regs[r0] = tag
                    self.lgkm = []
            elif op == "s_barrier":
                assert not self.lgkm, "a fragment read is still in flight at the barrier (its slot may be refilled behind it)"
                self.barriers.append(self.t)
            elif op == "ds_read_b128":
                m = re.match(r"v\[(\d+):(\d+)\]", a[0])
                r0 = int(m.group(1))
                assert int(m.group(2)) == r0 + 3
                reg = int(a[1].split()[0][1:])
                off = int(a[1].split("offset:")[1]) if "offset:" in a[1] else 0
                addr = self.v[reg] + off            # lane 0: row 0 of the fragment, chunk 4 h
                is_a = addr < B_BASE
                h = (addr >> 6) & 1
                assert reg == (gen.ADA288 if is_a else gen.ADB288) + h
                base, size, rows = (0, A_SLOT, 144) if is_a else (B_BASE, B_SLOT, 128)
                slot, o = divmod(addr - base, size)
                o -= ((self.w >> 1) if is_a else (self.w & 1)) * rows * 128 + (h << 6)
                frag = o // 2048
                assert o % 2048 == 0 and 0 <= frag < rows // 16
                tiles = set()
                for k in sorted({(addr - (h << 6)) // 4096, (addr - (h << 6) + 2047) // 4096}):       # 16 rows = two pieces
                    e = self.lds.get(k)
                    assert e is not None and k not in self.inflight, ("read of a piece that has not landed", l)
                    assert any(e["landed"] <= b <= self.t for b in self.barriers), ("read before the barrier behind its wait", l)
                    assert e["op"] == ("A" if is_a else "B") and e["group"] == (k * 4096 - base - slot * size) // 4096
                    tiles.add(e["tile"])
                    self.last_read[k] = self.t
                assert len(tiles) == 1
                for rr in range(r0, r0 + 4):
                    self.regs.pop(rr, None)
                self.lgkm.append((r0, ("A" if is_a else "B", tiles.pop(), h, frag)))
            elif op == "buffer_load_dwordx4":
                assert "lds" in l and self.m0_age >= 2, ("M0 written right in front of its LDS-DMA", l)
                vo = int(a[0][1:])
                is_a = a[1] == "RSA"
                base, n = (gen.VOA288, NPA) if is_a else (gen.VOB288, NPB)
                assert base <= vo < base + n
                # (piece i's voffset register holds i strides: the prologue's adds)
                assert self.v[vo] == (vo - base) * (1000000 if is_a else 2000000)
                soff = self.val(a[2].split()[0])
                st = self.stA if is_a else self.stB
                assert soff % st == 0
                self.dma("A" if is_a else "B", self.m0, soff // st, vo - base)
            elif op.startswith("v_mfma_f32_16x16x32"):
                ops_ = [x.strip() for x in rest.split(",")]
                assert ops_[0] == ops_[3], "accumulate in place"
                if ops_[0].startswith("a["):
                    n = int(re.match(r"a\[(\d+):(\d+)\]", ops_[0]).group(1))
                    acc = ((n // 4) // 8, (n // 4) % 8)
                    assert n % 4 == 0 and acc[0] < 8
                else:
                    acc = (8, int(re.fullmatch(r"%\[c(\d)\]", ops_[0]).group(1)))
                fb = int(re.match(r"v\[(\d+):", ops_[1]).group(1))
                fa = int(re.match(r"v\[(\d+):", ops_[2]).group(1))
                assert fa in self.regs and fb in self.regs, ("operand not in registers", l)
                self.mfma_log.append((acc, self.regs[fa], self.regs[fb]))
            else:
                raise AssertionError(f"unmodelled instruction: {l}")


@pytest.mark.parametrize("nk", [2, 3, 4, 5, 16])
@pytest.mark.parametrize("w", [0, 1, 2, 3])
@pytest.mark.parametrize("walk", [False, True])
def test_simulated_stream_is_consistent(nk, w, walk):
    sim = Sim(nk, w)
    wr, wc = w >> 1, w & 1
    sub = {"%[stA]": str(sim.stA), "%[stB]": str(sim.stB), "%[nk]": str(nk), "%[wv]": str(w * 1024), "%[iA]": "1000000",
           "%[iB]": "2000000", "%[voA]": "0", "%[voB]": "0", "%[adA]": str(wr * 144 * 128),
           "%[adB]": str(B_BASE + wc * 128 * 128), "%[rsB]": "RSB", "%[rsA]": "RSA", "@SFX@": "bf16", "%=": "X"}
    lines = []
    for l in gen.loop_text288(walk):
        for k, v in sub.items():
            l = l.replace(k, v)
        lines.append(l)
    assert gen.order_ok(lines)
    sim.run(lines)
    assert set(sim.requested) == {("A", t, i) for t in range(nk) for i in range(NPA)} | \
        {("B", t, i) for t in range(nk) for i in range(NPB)}
    assert not sim.vmq, "pieces still in flight at the end"
    assert not sim.lgkm
    # 144 MFMAs per K-tile; accumulator (i, j) <- A fragment i x B fragment j of tile T, k32-step h, each exactly once and
    # in ascending (T, h) per accumulator
    assert len(sim.mfma_log) == 144 * nk
    order = {}
    for n, (acc, pa, pb) in enumerate(sim.mfma_log):
        T, h = n // 144, (n % 144) // 72
        assert pa == ("A", T, h, acc[0]) and pb == ("B", T, h, acc[1]), (n, acc, pa, pb)
        order.setdefault(acc, []).append((T, h))
    assert len(order) == 72
    for acc, seq in order.items():
        assert seq == [(T, h) for T in range(nk) for h in range(2)], acc


def test_the_simulation_catches_a_protocol_error():
    """the checks above are live: a stream that requests A(T + 2) BEFORE tile T's barrier (a third slot would be needed) fails"""
    lines = gen.loop_text288(False)
    bar = [n for n, l in enumerate(lines) if l == "s_barrier"]
    first_a = next(n for n in range(bar[1], len(lines)) if "buffer_load_dwordx4" in lines[n] and "%[rsA]" in lines[n])
    moved = lines[:bar[1] - 1] + ["s_add_u32 s69, %[wv], s64", "s_mov_b32 m0, s69", "s_nop 0", lines[first_a]] + lines[bar[1] - 1:]
    sub = {"%[stA]": "128", "%[stB]": "128", "%[nk]": "4", "%[wv]": "0", "%[iA]": "1000000", "%[iB]": "2000000", "%[voA]": "0",
           "%[voB]": "0", "%[adA]": "0", "%[adB]": str(B_BASE), "%[rsB]": "RSB", "%[rsA]": "RSA", "@SFX@": "bf16", "%=": "X"}
    out = []
    for l in moved:
        for k, v in sub.items():
            l = l.replace(k, v)
        out.append(l)
    with pytest.raises(AssertionError):
        Sim(4, 0).run(out)
