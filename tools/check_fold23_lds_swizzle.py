"""Host brute force of the LDS bank conflicts of conv_wino24_kernel's V plane (csrc/conv_wino24.hip, NCQ = 4: chunks of 16 channels) for
the 32-tile (8 waves) and the 16-tile (HALF, 4 waves) workgroup: the transform's `ds_write_b32` of every wave and the A-operand
`ds_read_b128` of every wave, with the bank rules of gfx950 — 64 banks of 4 bytes; `ds_read_b128` is served in four 16-lane groups
{0-3,12-15,20-27}, {4-11,16-19,28-31}, {32-35,44-47,52-59}, {36-43,48-51,60-63} on bank (a/4) mod 64; `ds_write_b32` in two 32-lane
groups on bank (a/4) mod 32.  A position only adds a multiple of the plane size (512 or 256 floats: a multiple of 64 banks), so one
position stands for all.  Prints the worst multiplicity per access (1 = conflict-free) and exits non-zero if the 16-tile plane is worse
than the 32-tile one.  Result: stores conflict-free, A reads 2-way on BOTH planes — the XOR with (tile >> 2) & 3 spreads sixteen
CONSECUTIVE lanes over all banks, but the hardware's groups pair tiles 0-3 and 12-15 of one k group with tiles 4-11 of the next, and
tiles 0-3 (k group 0) and 4-7 (k group 1) land on the same 16-byte slots.  ((0, 2, 3, 1)[tile >> 2] in place of tile >> 2 would be
conflict-free; not changed here: the 8-wave kernels keep their instruction streams.)

    python tools/check_fold23_lds_swizzle.py
"""
import sys

B128_GROUPS = [list(range(0, 4)) + list(range(12, 16)) + list(range(20, 28)), list(range(4, 12)) + list(range(16, 20)) + list(range(28, 32)),
               list(range(32, 36)) + list(range(44, 48)) + list(range(52, 60)), list(range(36, 44)) + list(range(48, 52)) + list(range(60, 64))]
B32_GROUPS = [list(range(0, 32)), list(range(32, 64))]


def worst(addr_of_lane, groups, width, banks):
    """Largest number of distinct addresses on one bank within a lane group (addresses in floats, width floats per lane)."""
    w = 0
    for g in groups:
        hit = {}
        for lane in g:
            a = addr_of_lane(lane)
            for j in range(width):
                hit.setdefault((a + j) % banks, set()).add(a + j)
        w = max(w, max(len(v) for v in hit.values()))
    return w


def check(ntiles):
    nwaves = ntiles // 16 * 4
    res = {}
    # V store of the transform: thread tid -> (tile it = tid / 16, channel ik = tid % 16)
    def vdst(tid):
        it, ik = tid // 16, tid % 16
        return it * 16 + (((ik >> 2) ^ ((it >> 2) & 3)) << 2) + (ik & 3)
    assert sorted(vdst(t) for t in range(ntiles * 16)) == list(range(ntiles * 16))        # a permutation of the plane
    res["ds_write_b32"] = max(worst(lambda l, w=w: vdst(w * 64 + l), B32_GROUPS, 1, 32) for w in range(nwaves))
    # A operand of the MFMA: lane -> (tile th*16 + l15, k group ks)
    def aoff(th, lane):
        tile, ks = th * 16 + (lane & 15), lane >> 4
        return tile * 16 + ((ks ^ ((tile >> 2) & 3)) << 2)
    res["ds_read_b128"] = max(worst(lambda l, th=th: aoff(th, l), B128_GROUPS, 4, 64) for th in range(ntiles // 16))
    # the read returns what the store put there: lane (tile, ks) component j = channel ks*4 + j of that tile
    for th in range(ntiles // 16):
        for lane in range(64):
            tile, ks = th * 16 + (lane & 15), lane >> 4
            for j in range(4):
                assert aoff(th, lane) + j == vdst(tile * 16 + ks * 4 + j)
    return res


def main():
    res = {}
    for ntiles in (32, 16):
        res[ntiles] = r = check(ntiles)
        print("%d-tile plane (%d floats per position): %s" % (ntiles, ntiles * 16, ", ".join("%s %d-way" % kv for kv in sorted(r.items()))))
    return 1 if any(res[16][k] > res[32][k] for k in res[16]) else 0


if __name__ == "__main__":
    sys.exit(main())
