// Host check of the workgroup-wide traceback of vd_decode_pk's batched launches (vd_pk_wg.h, vd_kernel_pk.h
// "Batched"), through the functions the kernel itself calls.  A wave that ran fewer blocks or passes than its
// workgroup would skip a workgroup barrier and hang the launch, so the counts are argued here, on the CPU:
//  1. the four waves of a workgroup take their chunks from the same batch and from the eight chunks the block
//     count is computed for, so pk_wg_blocks is one value per workgroup;
//  2. it is the maximum over those chunks of (traced words + 2), and 0 only when all eight are empty;
//  3. the block loop and the pass schedule (staggered first pass, then every TBS blocks, then the last block)
//     run the same passes in every wave;
//  4. over a launch, the lane -> (wave, half, slot) map of the tracing wave emits every (chunk, word) exactly
//     once, never reads past the ring, and every wave takes its turn when there are four passes or more.
// Prints "ok" or the first failures.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "vd_kernel_pk.h"

using namespace vd;

static int fails = 0;
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            if (fails++ < 20) { printf("FAIL %s: ", #c); printf(__VA_ARGS__); printf("\n"); } \
        }                                                    \
    } while (0)

struct Pass {
    uint32_t j, kb, nw;
    bool operator==(const Pass& o) const { return j == o.j && kb == o.kb && nw == o.nw; }
};

// the kernel's block loop for one wave: groups of three blocks, block j ends the loop when j + 1 >= nblk
static std::vector<Pass> passes_of(uint32_t nblk, uint32_t wg, uint32_t tbs)
{
    std::vector<Pass> out;
    uint32_t kb = 0, tbn = pk_first_tbn(wg, tbs);
    for (uint32_t j = 0; nblk; j++) {
        if (pk_pass_at(j, kb, tbn, nblk)) {
            out.push_back(Pass{j, kb, j - 1 - kb});
            kb = j - 1;
            tbn = tbs;
        }
        if (!(j + 1 < nblk)) break;
    }
    return out;
}

static void check_launch(uint64_t packNum, int ob, uint32_t nbatch, uint32_t tbs)
{
    Geom g{};
    g.packNum = packNum;
    g.nchunks = kChunks;
    g.nbatch = nbatch;
    const uint32_t grid = (uint32_t)((uint64_t)kChunks * nbatch / (2 * kWaves));  // vd_plan.h, Form::PkBatched
    std::vector<uint8_t> emitted;
    for (uint32_t wg = 0; wg < grid; wg++) {
        const uint32_t c0 = pk_wg_chunk0(g, wg), nblk = pk_wg_blocks(g, wg, ob);
        // 1. the waves' own chunk indices (as the kernel computes them)
        uint32_t W[2 * kWaves], wmax = 0;
        for (uint32_t wv = 0; wv < (uint32_t)kWaves; wv++) {
            const uint32_t gc = 2u * (wg * kWaves + wv), batch = gc / g.nchunks, cA = gc - batch * g.nchunks;
            CHECK(batch == 2u * (wg * kWaves) / g.nchunks && batch < nbatch, "wg %u wave %u batch %u", wg, wv, batch);
            CHECK(cA == c0 + 2u * wv && cA + 1u < g.nchunks, "wg %u wave %u chunk %u first %u", wg, wv, cA, c0);
            // the tracing lanes find the same chunks from their own wave's cA
            for (uint32_t l = 0; l < 64; l++) {
                const PkTraceRole r = pk_trace_role(l);
                CHECK(cA - 2u * wv + 2u * r.wave + r.half == c0 + (l >> 3), "wg %u wave %u lane %u", wg, wv, l);
            }
            W[2 * wv] = pk_words32(chunk_range(g, cA).words, ob);
            W[2 * wv + 1] = pk_words32(chunk_range(g, cA + 1u).words, ob);
        }
        // 2. the maximum over the eight chunks
        for (uint32_t w : W) wmax = w > wmax ? w : wmax;
        CHECK(nblk == (wmax ? wmax + 2u : 0u), "pack %llu ob %d wg %u: blocks %u, longest chunk %u", (unsigned long long)packNum, ob, wg, nblk, wmax);
        // 3. every wave runs the same passes (each from the count it computes itself)
        const std::vector<Pass> ps = passes_of(nblk, wg, tbs);
        for (uint32_t wv = 1; wv < (uint32_t)kWaves; wv++)
            CHECK(passes_of(pk_wg_blocks(g, wg, ob), wg, tbs) == ps, "wg %u wave %u: another pass schedule", wg, wv);
        CHECK((nblk == 0) == ps.empty(), "wg %u: %u blocks, %zu passes", wg, nblk, ps.size());
        // 4. the tracing wave's lanes cover every word once
        emitted.assign(2 * kWaves * (size_t)(wmax + 1u), 0);
        uint32_t turns = 0;
        for (size_t n = 0; n < ps.size(); n++) {
            const Pass& p = ps[n];
            CHECK(p.nw >= 1u && p.nw <= tbs && tbs + 1u <= 8u, "wg %u pass %zu: %u words, ring of %u", wg, n, p.nw, tbs + 1u);
            turns |= 1u << (n % kWaves);  // the tracing wave
            for (uint32_t l = 0; l < 64; l++) {
                const PkTraceRole r = pk_trace_role(l);
                const uint32_t c = 2u * r.wave + r.half, k = p.kb + r.slot;
                if (r.slot < p.nw && k < W[c]) emitted[c * (size_t)(wmax + 1u) + k]++;
            }
        }
        for (uint32_t c = 0; c < 2u * kWaves; c++)
            for (uint32_t k = 0; k <= wmax; k++)
                CHECK(emitted[c * (size_t)(wmax + 1u) + k] == (k < W[c] ? 1 : 0), "pack %llu ob %d wg %u chunk %u word %u emitted %u times",
                      (unsigned long long)packNum, ob, wg, c, k, emitted[c * (size_t)(wmax + 1u) + k]);
        if (ps.size() >= (size_t)kWaves) CHECK(turns == 15u, "wg %u: tracing waves %x", wg, turns);
    }
}

int main()
{
    static_assert(PkLds<8>::TBS == 5 && PkLds<7>::TBS == 6, "the two pass lengths of the batched kernels");
    std::vector<uint64_t> packs;
    for (uint64_t p = 0; p <= 64; p++) packs.push_back(p);
    for (uint64_t w : {0, 1, 4, 5, 6, 7, 12})
        for (uint64_t r : {0, 1, 7, 8, 9, 4681, 6399})
            for (int d = -1; d <= 1; d++)
                if (6400 * w + r + d + 1 > 0) packs.push_back(6400 * w + r + d);
    size_t n = 0;
    for (uint64_t p : packs)
        for (int ob : {32, 16})
            for (uint32_t nb : {1u, 3u})
                for (uint32_t tbs : {(uint32_t)PkLds<8>::TBS, (uint32_t)PkLds<7>::TBS}) {
                    check_launch(p, ob, nb, tbs);
                    n++;
                }
    if (fails) {
        printf("%d failures in %zu launches\n", fails, n);
        return 1;
    }
    printf("ok\n");
    return 0;
}
