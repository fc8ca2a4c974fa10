// vd_pk_wg.h -- the workgroup-wide traceback of vd_decode_pk's batched launches: how many blocks a workgroup
// decodes, when its traceback passes fall and which lane of the tracing wave traces which word.  Pure
// functions of the geometry and the workgroup index, for the device and the host: everything that decides how
// many workgroup barriers a wave executes is here, and tests/cxx/pk_wg_blocks_check.cpp replays it on the CPU
// (a wave that ran one barrier fewer than its workgroup would hang the launch).
#pragma once
#include "vd_kernels.h"

namespace vd {

// 32-bit words traced for a chunk of `words` output words of ob bits (O_B16: each traced word is written as
// two 16-bit words, the last one possibly half)
__host__ __device__ constexpr uint32_t pk_words32(uint32_t words, int ob) { return ob == 32 ? words : (words + 1u) / 2u; }

// The first of the 2 kWaves chunks of workgroup wg inside its batch (launch chunk c = chunk c % nchunks of
// batch c / nchunks; the plan launches this form only when nchunks % (2 kWaves) == 0, so a workgroup never
// straddles a batch).
__host__ __device__ inline uint32_t pk_wg_chunk0(const Geom& g, uint32_t wg)
{
    return (2u * kWaves * wg) % g.nchunks;  // (32-bit as the kernel's own chunk index)
}

// Blocks every wave of workgroup wg decodes: its longest chunk's words + 2 (local word k is traced from
// blocks k + 1 and k + 2), 0 when all its chunks are empty.  Chunk lengths never grow with the chunk index
// (chunk_range: base + 1 below rem, base from there on), so the workgroup's first chunk is its longest.
__host__ __device__ inline uint32_t pk_wg_blocks(const Geom& g, uint32_t wg, int ob)
{
    const uint32_t w = pk_words32(chunk_range(g, pk_wg_chunk0(g, wg)).words, ob);
    return w ? w + 2u : 0u;
}

// Pass schedule.  Block j's ring words go to slot j - 1 - kb (kb: the block before slot 0's); a pass falls
// when the ring holds tbn words and their convergence block, and after the last block.  The first pass of
// workgroup wg is staggered (tbs: ring words per pass, PkLds::TBS), the later ones come every tbs blocks.
__host__ __device__ constexpr uint32_t pk_first_tbn(uint32_t wg, uint32_t tbs) { return tbs - (wg & 3u) % tbs; }
__host__ __device__ constexpr bool pk_pass_at(uint32_t j, uint32_t kb, uint32_t tbn, uint32_t nblk)
{
    return j >= 2u && (j - 1u - kb == tbn || j == nblk - 1u);
}

// Lane roles of the tracing wave: lane l traces ring slot l & 7 (a pass has at most PkLds::TBS <= 6 words per
// chunk, so slots 6 and 7 idle) of half (l >> 3) & 1 of wave l >> 4, i.e. of the workgroup's chunk l >> 3.
struct PkTraceRole {
    uint32_t wave, half, slot;
};
__host__ __device__ constexpr PkTraceRole pk_trace_role(uint32_t lane)
{
    return PkTraceRole{lane >> 4, (lane >> 3) & 1u, lane & 7u};
}
static_assert(kWaves * 16 == 64, "one tracing wave covers the workgroup: 16 lanes per wave, 8 per chunk");

}  // namespace vd
