"""CPU predictor of vd_split_redecodes for one segment launch of vd_decode_tg (test helper, no GPU).

It restates the launch's geometry (vd_segplan.h seg_table; vd_kernel_tg.h seg_bound, seg_run, seg_nruns) and
walks the kernel's pass loop (vd_kernel_tg.h "segment launches") on the oracle's metric vectors
(vd_oracle.block_vectors_flat: max only, renormalised to state 0, so independent of the tie rule, like the
kernel's comparison of renormalised vectors):

  * workgroup g decodes the chunks [t[g], t[g + 1]) of its table as 4 segments; segment q spans [b[q], b[q + 1])
    with b = seg_bound.  It is speculative iff b[q].a > 0: chunk i = b[q].i, boundary word a;
  * pass 0: a speculative segment's first run starts at chunk block s0 = a + 1 - warm from equal metrics; its
    start vector vS[q] is the vector after `warm` blocks (at the start of chunk block a + 1).  The left
    neighbour's end vector vE[q - 1] is its last run's vector at the start of the same chunk block a + 1; that run
    starts at the chunk start, or, when segment q - 1 is itself a speculative single-run segment of the same
    chunk, at that segment's own s0;
  * verified = {0} and the segments that start at a chunk start.  After each pass, for q = 1..3 in order, q
    becomes verified iff q - 1 is (already updated) and vS[q] == vE[q - 1].  All verified: the workgroup ends.
    Otherwise every unverified q adds 1 to the count, takes vIn = vE[q - 1] as the pass just finished left it,
    sets vS[q] = vIn and runs its first run again from chunk block a + 1; when that run holds the segment's
    right boundary (a single-run segment that ends inside the chunk) its vE[q] becomes the vector after the
    blocks a + 1 .. b_end of that decode, else vE[q] stays (its last run started at a chunk start: exact);
  * the first unverified segment always restarts from an exact vector, so there are at most 3 re-decode passes.
"""
import collections

import numpy as np

WAVES = 4      # vd_kernels.h kWaves
SEG_SNAP = 8   # vd_kernel_tg.h kSegSnap
WARM = 6       # vd_kernels.h Geom::segWarm
NCHUNKS = 6400  # vd_kernels.h kChunks
PIECES, THIRDS, SEVENTHS = 0, 1, 2  # vd_segplan.h SegMode
MODES = {"pieces": PIECES, "thirds": THIRDS, "sevenths": SEVENTHS}

Run = collections.namedtuple("Run", "i s0 words E Xspec Xcmp")
Prediction = collections.namedtuple("Prediction", "total hist spec_wgs chained passes mismatch0")
Prediction.__doc__ = """total: the launch's re-decode count; hist: {passes: workgroups} over the workgroups with a
speculative segment (1 = no re-decode); spec_wgs: their number; chained: the counted re-decodes whose start vector
already equalled the left neighbour's end vector and that ran only because that neighbour was unverified; passes:
passes per workgroup; mismatch0: the (workgroup, q) whose pass-0 start vector differs from the left end vector"""


def seg_table(nsimd, mode, nch=NCHUNKS):
    """vd_segplan.h seg_table: the first chunk of every workgroup, then the chunk count; [] = no table"""
    t = [0]
    if mode == SEVENTHS:
        if nsimd % 32 != 0:
            return []
        for g in range(7 * nsimd // 4):
            t.append(t[-1] + (4 if ((g // 8) % 7) % 2 == 0 else 3))
        return t if t[-1] == nch else []
    if mode == PIECES:
        rem = nch % nsimd
        nwhole = nch - rem
        if rem == 0 or rem * WAVES != nsimd or nch // nsimd + 1 > 8:
            return []
        t += list(range(WAVES, nwhole + 1, WAVES))
        t += list(range(nwhole + 1, nch + 1))
        return t
    nwg = 2 * nsimd
    if nch < 3 * nwg or nch - 3 * nwg != nwg // 8 or nwg % 256 != 0:
        return []
    for g in range(nwg):
        n = g // 8
        t.append(t[-1] + (4 if n // 32 == (n % 32) % 8 else 3))
    return t if t[-1] == nch else []


def launch_table(nsimd, mode):
    """the table a segment launch takes (vd_plan.h plan_launch): thirds and sevenths fall back to pieces"""
    return seg_table(nsimd, mode) or seg_table(nsimd, PIECES)


def chunk_words(vo, opt, input_num, nchunks=NCHUNKS):
    """32-bit words traced per chunk (the kernel's words32: O_B16 chunks of w 16-bit words trace (w + 1) / 2)"""
    bpp = 16 if (opt & 0xF00) == vo.O_B16 else 32
    pack = vo.message_len(opt, input_num) // bpp
    words = pack // nchunks + (np.arange(nchunks) < pack % nchunks)
    return words if bpp == 32 else (words + 1) // 2


def seg_bound(W, q):
    """vd_kernel_tg.h seg_bound: boundary q (0 .. 4) of a workgroup whose chunks have W[i] words, as (i, a)"""
    k = len(W)
    if q == 0:
        return 0, 0
    if q == WAVES:
        return k, 0
    cum = [0]
    for w in W:
        cum.append(cum[-1] + w)
    x = q * cum[k] // WAVES
    i = 0
    while i + 1 < k and cum[i + 1] <= x:
        i += 1
    a = x - cum[i]
    if a < SEG_SNAP:
        return i, 0
    if W[i] - a < SEG_SNAP:
        return i + 1, 0
    return i, a - (a + 1) % 3


def seg_nruns(b0, b1):
    return b1[0] - b0[0] + (1 if b1[1] != 0 else 0)


def seg_run(W, b0, b1, r, warm=WARM):
    """vd_kernel_tg.h seg_run"""
    i = b0[0] + r
    a = b0[1] if r == 0 else 0
    b = b1[1] if i == b1[0] else W[i]
    s0 = 0 if a == 0 else a + 1 - warm
    return Run(i, s0, b - s0, a - s0, -1 if a == 0 else a + 1 - s0, -1 if b == W[i] else b + 1 - s0)


def workgroups(table, words):
    """(c0, k, [5 bounds], [[runs of segment q]]) of every workgroup of a table over chunks of words[c] words"""
    out = []
    for g in range(len(table) - 1):
        c0, k = table[g], table[g + 1] - table[g]
        W = [int(w) for w in words[c0:c0 + k]]
        b = [seg_bound(W, q) for q in range(WAVES + 1)]
        runs = [[seg_run(W, b[q], b[q + 1], r) for r in range(seg_nruns(b[q], b[q + 1]))] for q in range(WAVES)]
        out.append((c0, k, b, runs))
    return out


def dump_lines(nsimd, mode, pack, o16):
    """the text tests/cxx/seg_runs_dump.cpp prints for (nsimd, mode, packNum, 16-bit output words)"""
    table = seg_table(nsimd, mode)
    if not table:
        return []
    words = pack // NCHUNKS + (np.arange(NCHUNKS) < pack % NCHUNKS)
    if o16:
        words = (words + 1) // 2
    lines = []
    for g, (c0, k, b, runs) in enumerate(workgroups(table, words)):
        lines.append(f"wg {g} c0 {c0} k {k} bounds " + " ".join(f"{i}:{a}" for i, a in b))
        for q in range(WAVES):
            for r, rg in enumerate(runs[q]):
                lines.append(f"run {g} {q} {r} {rg.i} {rg.s0} {rg.words} {rg.E} {rg.Xspec} {rg.Xcmp}")
    return lines


def predict(vo, opt, packed, input_num, table, nchunks=NCHUNKS, nthreads=16):
    """Prediction for one segment launch of `packed` (the packed words; float channel values of a fused launch and
    depunctured streams go through vo.pack first) with the segment table `table`."""
    W = chunk_words(vo, opt, input_num, nchunks)
    # speculative segments as flat arrays: workgroup, q, chunk, boundary word a, the start block of the left
    # neighbour's run that ends there, own end block (-1: the first run does not hold the right boundary)
    sg, sq, sc, sa, sl, se = [], [], [], [], [], []
    for g, (c0, k, b, runs) in enumerate(workgroups(table, W)):
        for q in range(1, WAVES):
            i, a = b[q]
            if a == 0:
                continue
            first, left = runs[q][0], runs[q - 1][-1]
            assert first.Xspec == WARM and first.s0 == a + 1 - WARM and first.s0 % 3 == 0
            assert left.i == i and left.Xcmp + left.s0 == a + 1, "no left end vector at the boundary block"
            assert left.s0 == 0 or (len(runs[q - 1]) == 1 and b[q - 1] == (i, left.s0 + WARM - 1))
            sg.append(g)
            sq.append(q)
            sc.append(c0 + i)
            sa.append(a)
            sl.append(left.s0)
            se.append(first.s0 + first.Xcmp - 1 if first.Xcmp >= 0 else -1)
    sg, sq, sc, sa, sl, se = (np.array(x, dtype=np.int64) for x in (sg, sq, sc, sa, sl, se))
    n = sg.size
    ngroups = len(table) - 1
    if n == 0:
        return Prediction(0, {}, 0, 0, np.ones(ngroups, np.int64), [])
    # slot of segment (g, q): its row in the flat arrays, -1 = not speculative (verified from the start)
    slot = np.full((ngroups, WAVES), -1, np.int64)
    slot[sg, sq] = np.arange(n)
    left_slot = slot[sg, sq - 1]  # >= 0: the left neighbour is speculative too

    def last_rows(jobs, start=None):
        has = None if start is None else np.ones(len(jobs), np.uint8)
        vec, row = vo.block_vectors_flat(opt, packed, input_num, jobs, start, has, nchunks=nchunks, nthreads=nthreads)
        return vec[row + jobs[:, 2] - 1]

    # pass 0: vS after the warm-up blocks; vEl = the left neighbour's end vector at the same block a + 1
    vS = last_rows(np.stack([sc, sa + 1 - WARM, np.full(n, WARM)], 1))
    vEl = last_rows(np.stack([sc, sl, sa + 1 - sl], 1))
    verified = np.zeros(n, bool)
    passes = np.ones(ngroups, np.int64)
    total = chained = 0
    mismatch0 = None
    for _ in range(WAVES):
        # the checks of q = 1..3 in order: the left neighbour's state as this same loop has updated it
        same = (vS == vEl).all(axis=1)
        if mismatch0 is None:
            mismatch0 = [(int(g), int(q)) for g, q in zip(sg[~same], sq[~same])]
        for q in range(1, WAVES):
            m = (sq == q) & ~verified
            lv = np.where(left_slot[m] >= 0, verified[np.maximum(left_slot[m], 0)], True)
            verified[m] = lv & same[m]
        bad = np.flatnonzero(~verified)
        if bad.size == 0:
            break
        total += bad.size
        chained += int(same[bad].sum())
        passes[np.unique(sg[bad])] += 1
        # the re-decode pass: every read is of the vectors the pass before left
        vin = vEl[bad].copy()
        vS[bad] = vin
        own = bad[se[bad] >= 0]  # re-runs that end at the segment's right boundary publish a new end vector
        if own.size:
            new = last_rows(np.stack([sc[own], sa[own] + 1, se[own] - sa[own]], 1), vS[own])
            right = slot[sg[own], np.minimum(sq[own] + 1, WAVES - 1)]
            ok = (sq[own] + 1 < WAVES) & (right >= 0)
            assert ok.all(), "a segment that ends inside a chunk has a speculative right neighbour"
            vEl[right] = new
    else:
        raise AssertionError("more than 3 re-decode passes")
    spec = np.unique(sg)
    hist = collections.Counter(passes[spec].tolist())
    return Prediction(total, dict(sorted(hist.items())), int(spec.size), chained, passes, mismatch0)
