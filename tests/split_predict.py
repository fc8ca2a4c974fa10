"""CPU predictor of vd_split_redecodes for one split launch of vd_decode_pk (test helper, no GPU).

It walks the kernel's pass loop (vd_kernel_pk.h "Split") on the oracle's metric vectors (vd_oracle.block_vectors:
max only, so independent of the tie rule, like the kernel's comparison of renormalised vectors):

  * chunk c has W(c) 32-bit words (O_B16: (words + 1) / 2, the kernel's WA) and is cut at pk_cut(p, P, W);
  * the first nchunks - tail chunks are whole-chunk waves with P = 2, the last `tail` chunks tail workgroups with
    P = 8, wave q owning parts 2q and 2q + 1;
  * pass 0 runs every part from equal metrics, part 0 from the chunk start, part p from kPkWarm blocks before
    cut(p); part p's start vector is its vector at block cut(p) - 1, part p's end vector the one at block
    cut(p + 1) - 1;
  * each later pass runs again, from block cut(p) with the left neighbour's current end vector, every part p
    whose start vector differs from that end vector (all comparisons of a pass use the vectors the pass before
    left), and the kernel adds one count per such part (`atomicAdd(geo.stats, mA + mB)`);
  * early stops (vd_kernel_pk.h "Early stop") change neither the count nor the end vectors: a stopped re-decode
    has met the run whose end vector stands (tools/split_model.py asserts it).
"""
import collections

import numpy as np

K_WARM = 6  # vd_kernel_pk.h kPkWarm
WAVES = 4   # waves per workgroup (kWaves): a tail workgroup cuts its chunk into 2 * WAVES parts

Prediction = collections.namedtuple(
    "Prediction", "total passes whole_fail tail_redecodes both_halves tail_hist")
Prediction.__doc__ = """total: the launch's re-decode count; passes: passes per chunk (1 = no re-decode);
whole_fail: whole-chunk waves whose speculative start failed; tail_redecodes: the count's share from tail
workgroups; both_halves: (wave, pass) pairs of tail workgroups in which both halves re-decode; tail_hist:
{passes: tail chunks}"""


def pk_cut(p, P, W):
    """vd_kernel_pk.h pk_cut"""
    if p == 0:
        return 0
    if p >= P:
        return W
    return K_WARM + 3 * ((2 * p * (W - K_WARM) + 3 * P) // (6 * P))


def default_tail(multi_processor_count, nchunks=6400):
    """the tail chunks of the default launch: vd_plan.h plan_launch, nchunks mod nsimd with nsimd = 4 CUs"""
    return nchunks % (4 * multi_processor_count)


def chunk_words(vo, opt, input_num, nchunks=6400):
    """32-bit words traced per chunk (the kernel's WA)"""
    bpp = 16 if (opt & 0xF00) == vo.O_B16 else 32
    pack = vo.message_len(opt, input_num) // bpp
    words = pack // nchunks + (np.arange(nchunks) < pack % nchunks)
    return words if bpp == 32 else (words + 1) // 2


def numpy_branch_metrics(opt, packed, nstages):
    """[stage, label] branch metrics (-A, -B, B, A: tools/split_model.py's layout) of HARD or SOFT8 packed words,
    read with numpy alone -- the CPU tests' check of the oracle's bm_at and stage indexing"""
    be = np.ascontiguousarray(packed).view(np.uint32).astype(">u4").view(np.uint8)  # most significant byte first
    if (opt & 0xF) == 0:  # HARD: stage g is bits 31 - 2 (g % 16), 30 - 2 (g % 16) of word g / 16; BM = 1 - mismatches
        r = np.unpackbits(be)[:2 * nstages].reshape(-1, 2).astype(np.int64)
        A = 1 - ((r[:, 0] ^ 1) + (r[:, 1] ^ 1))
        B = 1 - ((r[:, 0] ^ 1) + r[:, 1])
    elif (opt & 0xF) == 2:  # SOFT8: stage g is the byte pair g of the most-significant-first byte stream
        s = be.view(np.int8)[:2 * nstages].reshape(-1, 2).astype(np.int64)
        A, B = s[:, 0] + s[:, 1], s[:, 0] - s[:, 1]
    else:
        raise ValueError("HARD and SOFT8 only")
    return np.stack([-A, -B, B, A], 1)


def split_model():
    """tools/split_model.py, the host model of the pass loop"""
    import os
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import split_model
    return split_model


def model_chunk(opt, packed, nbits, nchunks, c):
    """tools/split_model.py's Chunk over chunk c's stages of a HARD or SOFT8 packed input of nbits stages"""
    sm = split_model()
    bpp = 16 if (opt & 0xF00) == 0x100 else 32
    base, rem = divmod((nbits - 64) // bpp, nchunks)
    words, start = base + (c < rem), base * c + min(c, rem)
    ch = sm.Chunk.__new__(sm.Chunk)  # (its constructor draws an input of its own)
    ch.W = words if bpp == 32 else (words + 1) // 2
    ch.bm = numpy_branch_metrics(opt, packed, nbits)[bpp * start:bpp * start + 32 * (ch.W + 2)]
    return ch


def predict(vo, opt, packed, input_num, tail, nchunks=6400, nthreads=16):
    """Prediction for one split launch of `packed` (the packed words; float channel values of a fused launch go
    through vo.pack first) with the last `tail` chunks in tail workgroups."""
    assert 0 <= tail <= nchunks
    W = chunk_words(vo, opt, input_num, nchunks)
    assert W.min() >= 3 * K_WARM, "not a split launch"
    P = np.where(np.arange(nchunks) >= nchunks - tail, 2 * WAVES, 2)
    # parts as flat arrays: chunk, part index, cut(p), cut(p + 1), last part of its chunk
    pc, pp, c0, c1 = [], [], [], []
    for c in range(nchunks):
        for p in range(P[c]):
            pc.append(c)
            pp.append(p)
            c0.append(pk_cut(p, P[c], W[c]))
            c1.append(pk_cut(p + 1, P[c], W[c]))
    pc, pp, c0, c1 = (np.array(a, dtype=np.int64) for a in (pc, pp, c0, c1))
    n = pc.size
    first = pp == 0
    last = pp == P[pc] - 1
    # pass 0: part 0 over [0, cut(1)); part p over [cut(p) - 6, cut(p + 1)), the last part only up to its cut
    o = np.where(first, 0, c0 - K_WARM)
    stop = np.where(last & ~first, c0, c1)
    vec, row = vo.block_vectors_flat(opt, packed, input_num, np.stack([pc, o, stop - o], 1), nchunks=nchunks,
                                     nthreads=nthreads)
    sv = np.zeros((n, 64), np.int32)
    ev = np.zeros((n, 64), np.int32)
    sv[~first] = vec[(row + c0 - 1 - o)[~first]]
    ev[~last] = vec[(row + c1 - 1 - o)[~last]]
    del vec
    passes = np.ones(nchunks, np.int64)
    total = whole_fail = tail_re = both = 0
    idx = np.arange(n)
    while True:
        bad = idx[~first & (sv != np.roll(ev, 1, axis=0)).any(axis=1)]
        if bad.size == 0:
            break
        assert passes.max() < 2 * P.max(), "the kernel's pass cap would bind"
        total += bad.size
        passes[np.unique(pc[bad])] += 1
        in_tail = P[pc[bad]] > 2
        whole_fail += int((~in_tail).sum())
        tail_re += int(in_tail.sum())
        # halves 2q, 2q + 1 of one wave both re-decoding (whole-chunk waves: part 0 never does)
        tb = bad[in_tail]
        both += int(np.intersect1d(tb[pp[tb] % 2 == 0] + 1, tb).size)
        sv[bad] = ev[bad - 1]
        run = bad[~last[bad]]  # the last part's re-decode leaves no end vector
        if run.size:
            vec, row = vo.block_vectors_flat(opt, packed, input_num, np.stack([pc[run], c0[run], (c1 - c0)[run]], 1),
                                             ev[run - 1], np.ones(run.size, np.uint8), nchunks=nchunks,
                                             nthreads=nthreads)
            ev[run] = vec[row + (c1 - c0)[run] - 1]
    hist = collections.Counter(passes[nchunks - tail:].tolist()) if tail else {}
    return Prediction(total, passes, whole_fail, tail_re, both, dict(sorted(hist.items())))
