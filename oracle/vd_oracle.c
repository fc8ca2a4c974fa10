/*
 * vd_oracle.c -- CPU restatement of the reference decode path (TEST INFRASTRUCTURE ONLY).
 *
 * ORACLE / CHECKER.  Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library, and only to check (or time, as the reported CPU baseline) the HIP product
 * path.  The product (gpu-accelerated-viterbi-decoder_amd/) never links, loads or calls it.
 *
 * What it restates (reference = alireza-md93/GPU-Accelerated-Viterbi-Decoder, read as text only;
 * the reference cannot be built here: CUDA-only, and running a host emulation of it was refused
 * by the environment -- see SURVEY.md 8(c)):
 *   - option bitmask + size helpers ........ src/viterbi/viterbi.h:7-41,61-87, viterbi.cu:63-100
 *   - chunk partition (6400 chunks) ......... src/viterbi/viterbi.cu:19,156-165
 *   - branch metrics per input format ....... src/viterbi/viterbiBM.cuh:15-185
 *   - ACS, per-core tie rules ............... src/viterbi/viterbiACS.cuh:113-157,173-303,452-518
 *   - PM normalisation schedule (range check) src/viterbi/viterbiACS.cuh:307-378, viterbi.cu:173
 *   - traceback from state 0 ................ src/viterbi/viterbiTB.cuh:4-21, viterbi.cu:176-206
 *   - harness: bits/encoder/AWGN/packer/BER . src/viterbiDF.h:20-167, src/main.cpp:119-172
 *
 * Parity pinning: the known-answer BEN table and SHA-256 pins of SURVEY.md 8(c) (captured from a
 * host emulation of the reference's own kernel source before the refusal).  tests/test_oracle.py
 * checks this file against every one of them.
 *
 * Arithmetic: path metrics are int64 here, so there is no overflow; the reference's int16/int32/fp16
 * metrics are exact for every valid option combination (no overflow, integers < 2048 in fp16),
 * which vo_decode re-checks by emulating the reference's normalisation schedule and reporting
 * any range violation (then the restatement would no longer be authoritative).
 *
 * Build: oracle/Makefile (gcc -O2 -ffp-contract=off).
 */
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <pthread.h>

/* ---- option bitmask (viterbi.h:7-20) ---- */
enum { CH_HARD = 0, CH_SOFT4 = 1, CH_SOFT8 = 2, CH_SOFT16 = 3, CH_FP32 = 4 };
enum { M_B32 = 0, M_B16 = 1, M_FP16 = 2 };
enum { O_B32 = 0, O_B16 = 1 };
#define CH(o)   ((o) & 0xF)
#define MET(o)  (((o) >> 4) & 0xF)
#define OUT(o)  (((o) >> 8) & 0xF)
#define COMP(o) (((o) >> 12) & 0xF)

#define CL 7
#define POLY0 0171
#define POLY1 0133
#define NCHUNKS_REF 6400 /* viterbi.cu:19 blocksNum_total = 16*400 */

/* viterbi.h:22-41 */
int vo_options_valid(int o)
{
    int ch = CH(o), me = MET(o), out = OUT(o), cm = COMP(o);
    if (ch > CH_FP32 || me > M_FP16 || out > O_B16 || cm > 1) return 0;
    if (o & ~0xFFFF) return 0;
    if (ch == CH_SOFT8 && me == M_FP16) return 0;
    if (ch == CH_SOFT16 && me == M_FP16) return 0;
    if (ch == CH_SOFT16 && me == M_B16) return 0;
    if (me == M_FP16 && cm == 1) return 0;
    return 1;
}

static int bits_per_pack(int o) { return OUT(o) == O_B16 ? 16 : 32; }
/* extraL = roundup(32,bpp)-6 = 26, extraR = roundup(32,bpp)+6 = 38 for both bpp (viterbi.h:73-76) */
#define EXTRA_L 26
#define EXTRA_R 38

/* viterbi.cu:63-84 */
size_t vo_input_size(int o, size_t n)
{
    switch (CH(o)) {
    case CH_HARD:   return ((n + 7) / 8 * 8) / 8;
    case CH_SOFT4:  return ((n + 1) / 2 * 2) / 2;
    case CH_SOFT8:  return n;
    case CH_SOFT16: return n * 2;
    case CH_FP32:   return n * 4;
    }
    return 0;
}
/* viterbi.cu:86-92 (size_t arithmetic: underflows for n/2 < 64 exactly like the reference) */
size_t vo_message_len(int o, size_t n)
{
    size_t bpp = (size_t)bits_per_pack(o);
    return (n / 2 - (EXTRA_L + EXTRA_R)) / bpp * bpp;
}
size_t vo_output_size(int o, size_t n) { return vo_message_len(o, n) / 8; }

/* ---- branch metrics (viterbiBM.cuh) ----
 * For global stage g this returns A = BM[3] (labels o0=1,o1=1) and B = BM[2] (o0=1,o1=0);
 * BM[0] = -A and BM[1] = -B for every format (flipping both code bits negates the correlation). */
typedef struct {
    int ch;
    const uint32_t* w; /* packed words */
    const float* f;    /* FP32 */
    size_t nstages;    /* stages actually present in the buffer */
} bm_src;

static inline int sext(uint32_t v, int bits) { return (int)(v << (32 - bits)) >> (32 - bits); }

static void bm_at(const bm_src* s, size_t g, int* A, int* B)
{
    if (g >= s->nstages) {
        /* out-of-buffer read (only reachable by the O_B16 overrun, see vo_decode); the reference
         * reads whatever lies past its allocation -- defined here as zero words / 0.0f */
        if (s->ch == CH_HARD) { *A = -1; *B = 0; } /* r0=r1=0 */
        else { *A = 0; *B = 0; }
        return;
    }
    switch (s->ch) {
    case CH_HARD: { /* viterbiBM.cuh:15-40: word g>>4, bits 31-2(g%16), 30-2(g%16); BM = 1-#mismatch */
        uint32_t w = s->w[g >> 4];
        int sh = 31 - 2 * (int)(g & 15);
        int r0 = (w >> sh) & 1, r1 = (w >> (sh - 1)) & 1;
        *A = 1 - ((r0 ^ 1) + (r1 ^ 1)); /* L=3 */
        *B = 1 - ((r0 ^ 1) + (r1 ^ 0)); /* L=2 */
        return;
    }
    case CH_SOFT4: { /* viterbiBM.cuh:45-75: byte g%4 from MSB, hi nibble s0, lo nibble s1 */
        uint32_t w = s->w[g >> 2];
        uint32_t by = (w >> (24 - 8 * (int)(g & 3))) & 0xFF;
        int s0 = sext(by >> 4, 4), s1 = sext(by & 0xF, 4);
        *A = s0 + s1; *B = s0 - s1; return;
    }
    case CH_SOFT8: { /* viterbiBM.cuh:79-100: word g/2, even g -> bytes 3,2 ; odd -> bytes 1,0 */
        uint32_t w = s->w[g >> 1];
        int s0, s1;
        if ((g & 1) == 0) { s0 = sext(w >> 24, 8); s1 = sext((w >> 16) & 0xFF, 8); }
        else { s0 = sext((w >> 8) & 0xFF, 8); s1 = sext(w & 0xFF, 8); }
        *A = s0 + s1; *B = s0 - s1; return;
    }
    case CH_SOFT16: { /* viterbiBM.cuh:104-124: hi16 = s0, lo16 = s1 */
        uint32_t w = s->w[g];
        int s0 = sext(w >> 16, 16), s1 = sext(w & 0xFFFF, 16);
        *A = s0 + s1; *B = s0 - s1; return;
    }
    case CH_FP32: { /* viterbiBM.cuh:128-153: clamp to [-8,7], (int)(+-x0 +- x1) (truncation) */
        float x0 = s->f[2 * g], x1 = s->f[2 * g + 1];
        x0 = fminf(fmaxf(x0, -8.0f), 7.0f);
        x1 = fminf(fmaxf(x1, -8.0f), 7.0f);
        float a = x0 + x1, b = x0 - x1;
        *A = (int)a; *B = (int)b; return;
    }
    }
    *A = 0; *B = 0;
}

/* trellis tables: for new state T and predecessor bit b, old state O and label L */
static int g_tab_init = 0;
static int tabO[64][2], tabL[64][2];
static int parity7(int v) { v &= 0x7F; v ^= v >> 4; v ^= v >> 2; v ^= v >> 1; return v & 1; }
static void init_tabs(void)
{
    if (g_tab_init) return;
    for (int T = 0; T < 64; T++)
        for (int b = 0; b < 2; b++) {
            int R = (T << 1) | b; /* bit6 = newest input (u), bit0 = dropped bit b */
            tabO[T][b] = ((T & 31) << 1) | b;
            tabL[T][b] = (parity7(R & POLY0) << 1) | parity7(R & POLY1);
        }
    g_tab_init = 1;
}

/* per-core normalisation schedule (viterbi.cu:173, viterbiACS.cuh:307-378) */
static int chn_width(int ch)
{
    switch (ch) { case CH_HARD: return 1; case CH_SOFT4: return 4; case CH_SOFT8: return 8;
                  case CH_SOFT16: return 16; default: return 4; }
}

typedef struct {
    int opt;
    bm_src src;
    size_t nchunks;
    size_t packNum, base, rem;
    int bpp;
    void* out;
    int policy;        /* O_B16 overrun: 0 = a chunk's own words win, 1 = overrun words win */
    int* range_bad;    /* set when a metric leaves the reference's exact range */
    /* O_B16 overrun words are collected per chunk: [chunk][2] (value, valid) */
    uint16_t* ovf;
    uint8_t* ovf_valid;
} job_t;

/* decode one chunk; returns 0 on success */
static int decode_chunk(job_t* J, size_t c, uint64_t* dec /* scratch >= nst */, int* range_bad)
{
    const int o = J->opt, me = MET(o);
    const int bpp = J->bpp;
    size_t words = J->base + (c < J->rem ? 1 : 0);
    size_t startWord = J->base * c + (c < J->rem ? c : J->rem);
    size_t decLen = words * (size_t)bpp;
    size_t start = startWord * (size_t)bpp;
    if (words == 0) return 0;

    int tail16 = (bpp == 16) && (decLen % 32 == 16);
    size_t nst = 64 + (decLen + 31) / 32 * 32 + (tail16 ? 16 : 0);

    /* reference-faithful range tracking */
    int stride_log = (me == M_B16 ? 16 : me == M_B32 ? 32 : 11) - chn_width(CH(o)) - 2;
    long long stride = 1LL << stride_log;
    long long thr = me == M_B16 ? 16000 : me == M_B32 ? 1000000000LL : 500;
    long long lim = me == M_B16 ? 32767 : me == M_B32 ? 2147483647LL : 2048;

    long long pm[64], pn[64];
    for (int i = 0; i < 64; i++) pm[i] = 0;
    for (size_t t = 0; t < nst; t++) {
        int A, B;
        bm_at(&J->src, start + t, &A, &B);
        long long bm[4] = { -A, -B, B, A };
        int k = (int)(t % 6);
        uint64_t d = 0;
        for (int T = 0; T < 64; T++) {
            int u = T >> 5;
            long long c0 = pm[tabO[T][0]] + bm[tabL[T][0]];
            long long c1 = pm[tabO[T][1]] + bm[tabL[T][1]];
            if (c0 > lim || c0 < -lim || c1 > lim || c1 < -lim) *range_bad = 1;
            int pick;
            if (c1 > c0) pick = 1;
            else if (c1 < c0) pick = 0;
            else { /* tie rules: b32 k==0 -> 1 else !u ; b16 -> !u ; f16 -> u */
                if (me == M_B32) pick = (k == 0) ? 1 : !u;
                else if (me == M_B16) pick = !u;
                else pick = u;
            }
            pn[T] = pick ? c1 : c0;
            d |= (uint64_t)pick << T;
        }
        memcpy(pm, pn, sizeof(pm));
        dec[t] = d;
        if ((long long)(t % (size_t)stride) == 0) {
            long long mx = pm[0], mn = pm[0];
            for (int i = 1; i < 64; i++) { if (pm[i] > mx) mx = pm[i]; if (pm[i] < mn) mn = pm[i]; }
            if (mx > thr) for (int i = 0; i < 64; i++) pm[i] -= mn;
        }
    }

    /* traceback: word over stages [e-63, e-32] traced from state 0 at stage e */
    if (bpp == 32) {
        uint32_t* out = (uint32_t*)J->out + startWord;
        for (size_t k = 0; k < words; k++) {
            size_t e = 95 + 32 * k;
            int s = 0;
            for (size_t t = e; t > e - 32; t--) s = ((s & 31) << 1) | (int)((dec[t] >> s) & 1);
            uint32_t w = 0;
            for (int i = 0; i < 32; i++) {
                size_t t = e - 32 - (size_t)i;
                int b = (int)((dec[t] >> s) & 1);
                w |= (uint32_t)b << i;
                s = ((s & 31) << 1) | b;
            }
            out[k] = w;
        }
    } else {
        uint16_t* out = (uint16_t*)J->out;
        size_t nslides = (decLen + 31) / 32; /* full slides incl. the one that overruns */
        for (size_t k = 0; k < nslides; k++) {
            size_t e = 95 + 32 * k;
            int s = 0;
            for (size_t t = e; t > e - 32; t--) s = ((s & 31) << 1) | (int)((dec[t] >> s) & 1);
            uint32_t w = 0;
            for (int i = 0; i < 32; i++) {
                size_t t = e - 32 - (size_t)i;
                int b = (int)((dec[t] >> s) & 1);
                w |= (uint32_t)b << i;
                s = ((s & 31) << 1) | b;
            }
            size_t wi = 2 * k; /* chunk-relative 16-bit word index of the high half */
            out[startWord + wi] = (uint16_t)(w >> 16);
            if (wi + 1 < words) out[startWord + wi + 1] = (uint16_t)(w & 0xFFFF);
            else { J->ovf[2 * c + 0] = (uint16_t)(w & 0xFFFF); J->ovf_valid[2 * c + 0] = 1; }
        }
        if (tail16) {
            /* viterbi.cu:199-206 after the slide loop exited with slide = decLen + 16 */
            size_t e = decLen + 16 + 64 + 15;
            int s = 0;
            for (size_t t = e; t > e - 32; t--) s = ((s & 31) << 1) | (int)((dec[t] >> s) & 1);
            uint32_t w = 0;
            for (int i = 0; i < 16; i++) {
                size_t t = e - 32 - (size_t)i;
                int b = (int)((dec[t] >> s) & 1);
                w |= (uint32_t)b << i;
                s = ((s & 31) << 1) | b;
            }
            J->ovf[2 * c + 1] = (uint16_t)w; J->ovf_valid[2 * c + 1] = 1;
        }
    }
    (void)range_bad;
    return 0;
}

typedef struct { job_t* J; size_t c0, c1; int bad; } thr_arg;

static void* worker(void* p)
{
    thr_arg* a = (thr_arg*)p;
    size_t maxw = a->J->base + 1;
    size_t nst_max = 64 + (maxw * (size_t)a->J->bpp + 31) / 32 * 32 + 16 + 64;
    uint64_t* dec = (uint64_t*)malloc(nst_max * sizeof(uint64_t));
    if (!dec) { a->bad = 2; return NULL; }
    for (size_t c = a->c0; c < a->c1; c++) decode_chunk(a->J, c, dec, &a->bad);
    free(dec);
    return NULL;
}

/*
 * Decode `inputNum` encoded values (the reference's `run` argument) from `in` (encPack_t array)
 * into `out` (decPack_t array, vo_output_size bytes).  nchunks: 6400 reproduces the reference.
 * O_B16 overrun policy (the reference's cross-chunk write race):
 *   0 = every chunk's own words win (chunks retired in index order),
 *   1 = overrun words win (written last).
 * Returns 0 on success, 1 if a metric left the reference's exact range, <0 on bad arguments.
 */
int vo_decode_ex(int opt, const void* in, void* out, size_t inputNum, int nchunks, int policy, int nthreads,
                 size_t availStages);
int vo_decode(int opt, const void* in, void* out, size_t inputNum, int nchunks, int policy, int nthreads)
{
    return vo_decode_ex(opt, in, out, inputNum, nchunks, policy, nthreads, 0);
}
/* availStages != 0: number of stages readable in `in` (may exceed inputNum/2: models what the
 * reference's O_B16 overrun reads past the end of its input window) */
int vo_decode_ex(int opt, const void* in, void* out, size_t inputNum, int nchunks, int policy, int nthreads,
                 size_t availStages)
{
    if (!vo_options_valid(opt)) return -1;
    if (inputNum / 2 < EXTRA_L + EXTRA_R) return -2;
    if (nchunks <= 0) nchunks = NCHUNKS_REF;
    if (nthreads <= 0) nthreads = 1;
    init_tabs();
    job_t J;
    memset(&J, 0, sizeof(J));
    J.opt = opt;
    J.src.ch = CH(opt);
    J.src.w = (const uint32_t*)in;
    J.src.f = (const float*)in;
    J.src.nstages = inputNum / 2;
    if (CH(opt) == CH_HARD) { size_t nw = vo_input_size(opt, inputNum) / 4; if (J.src.nstages > nw * 16) J.src.nstages = nw * 16; }
    if (availStages) J.src.nstages = availStages;
    J.bpp = bits_per_pack(opt);
    size_t msg = vo_message_len(opt, inputNum);
    J.packNum = msg / (size_t)J.bpp;
    J.nchunks = (size_t)nchunks;
    J.base = J.packNum / J.nchunks;
    J.rem = J.packNum % J.nchunks;
    J.out = out;
    J.policy = policy;
    if (J.bpp == 16) {
        J.ovf = (uint16_t*)calloc(2 * J.nchunks, sizeof(uint16_t));
        J.ovf_valid = (uint8_t*)calloc(2 * J.nchunks, 1);
    }
    int bad = 0;
    pthread_t th[64];
    thr_arg args[64];
    if (nthreads > 64) nthreads = 64;
    size_t per = (J.nchunks + (size_t)nthreads - 1) / (size_t)nthreads;
    int nt = 0;
    for (int i = 0; i < nthreads; i++) {
        size_t c0 = per * (size_t)i, c1 = c0 + per;
        if (c1 > J.nchunks) c1 = J.nchunks;
        if (c0 >= c1) break;
        args[i].J = &J; args[i].c0 = c0; args[i].c1 = c1; args[i].bad = 0;
        nt++;
    }
    if (nt == 1) worker(&args[0]);
    else {
        for (int i = 0; i < nt; i++) pthread_create(&th[i], NULL, worker, &args[i]);
        for (int i = 0; i < nt; i++) pthread_join(th[i], NULL);
    }
    for (int i = 0; i < nt; i++) if (args[i].bad) bad = args[i].bad;
    if (J.bpp == 16) {
        uint16_t* o16 = (uint16_t*)out;
        size_t nwords = msg / 16;
        for (size_t c = 0; c < J.nchunks; c++) {
            size_t words = J.base + (c < J.rem ? 1 : 0);
            size_t startWord = J.base * c + (c < J.rem ? c : J.rem);
            for (int j = 0; j < 2; j++) {
                if (!J.ovf_valid[2 * c + j]) continue;
                size_t gi = startWord + words + (size_t)j;
                if (gi >= nwords) continue;          /* past the output buffer: dropped */
                /* the word belongs to a later chunk; policy decides who wins */
                /* policy 2: overrun wins only inside one reference thread block (chunks 2b, 2b+1
                 * share block b: its two warps run concurrently, blocks retire in order) */
                int wins = (policy == 1) || (policy == 2 && (c & 1) == 0);
                if (policy >= 16) { /* experimental bitmask: bit j = overrun word j wins; bit 2: even chunks only */
                    wins = (policy >> j) & 1;
                    if ((policy & 4) && (c & 1)) wins = 0;
                }
                if (wins) o16[gi] = J.ovf[2 * c + j];
            }
        }
        free(J.ovf); free(J.ovf_valid);
    }
    return bad == 2 ? -3 : (bad ? 1 : 0);
}

/*
 * Metric vectors at block ends (for the split launches' re-decode predictor, tests/split_predict.py).
 * Job j = (chunk, first block, block count): the add-compare-select recursion (max only: no tie rule, no
 * traceback, no normalisation schedule) over blocks first .. first + count - 1 of 32 stages each, block b of
 * chunk c starting at stage startWord(c) * bpp + 32 b, from equal metrics or, where has_start[j] is set, from
 * start[64 j ..].  After each block the 64 metrics renormalised to state 0 (pm[i] - pm[0]) are appended to
 * `out` (64 int32 per block, jobs in order).  Equal renormalised vectors mean equal decisions from there on
 * whatever the tie rule, which is what vd_decode_pk's split launch compares.
 * Returns 0, or <0 on bad arguments (a job's chunk out of range).
 */
typedef struct {
    const bm_src* src;
    size_t base, rem;
    int bpp;
    const uint32_t* jobs;
    const int32_t* start;
    const uint8_t* has_start;
    const size_t* off; /* first output block of each job */
    int32_t* out;
    size_t j0, j1;
} bv_arg;

static void* bv_worker(void* p)
{
    bv_arg* a = (bv_arg*)p;
    for (size_t j = a->j0; j < a->j1; j++) {
        size_t c = a->jobs[3 * j], b0 = a->jobs[3 * j + 1], nb = a->jobs[3 * j + 2];
        size_t startWord = a->base * c + (c < a->rem ? c : a->rem);
        size_t g = startWord * (size_t)a->bpp + 32 * b0;
        long long pm[64], pn[64];
        for (int i = 0; i < 64; i++) pm[i] = a->has_start && a->has_start[j] ? a->start[64 * j + (size_t)i] : 0;
        int32_t* o = a->out + 64 * a->off[j];
        for (size_t b = 0; b < nb; b++) {
            for (int t = 0; t < 32; t++, g++) {
                int A, B;
                bm_at(a->src, g, &A, &B);
                long long bm[4] = { -A, -B, B, A };
                for (int T = 0; T < 64; T++) {
                    long long c0 = pm[tabO[T][0]] + bm[tabL[T][0]];
                    long long c1 = pm[tabO[T][1]] + bm[tabL[T][1]];
                    pn[T] = c1 > c0 ? c1 : c0;
                }
                memcpy(pm, pn, sizeof(pm));
            }
            for (int i = 63; i >= 0; i--) pm[i] -= pm[0];
            for (int i = 0; i < 64; i++) o[64 * b + (size_t)i] = (int32_t)pm[i];
        }
    }
    return NULL;
}

int vo_block_vectors(int opt, const void* in, size_t inputNum, int nchunks, size_t njobs, const uint32_t* jobs,
                     const int32_t* start, const uint8_t* has_start, int32_t* out, int nthreads)
{
    if (!vo_options_valid(opt)) return -1;
    if (inputNum / 2 < EXTRA_L + EXTRA_R) return -2;
    if (nchunks <= 0) nchunks = NCHUNKS_REF;
    if (nthreads <= 0) nthreads = 1;
    if (nthreads > 64) nthreads = 64;
    if (has_start && !start) return -4;
    for (size_t j = 0; j < njobs; j++) if (jobs[3 * j] >= (uint32_t)nchunks) return -5;
    if (njobs == 0) return 0;
    init_tabs();
    bm_src src;
    src.ch = CH(opt);
    src.w = (const uint32_t*)in;
    src.f = (const float*)in;
    src.nstages = inputNum / 2;
    if (CH(opt) == CH_HARD) { size_t nw = vo_input_size(opt, inputNum) / 4; if (src.nstages > nw * 16) src.nstages = nw * 16; }
    int bpp = bits_per_pack(opt);
    size_t packNum = vo_message_len(opt, inputNum) / (size_t)bpp;
    size_t* off = (size_t*)malloc(njobs * sizeof(size_t));
    if (!off) return -3;
    size_t tot = 0;
    for (size_t j = 0; j < njobs; j++) { off[j] = tot; tot += jobs[3 * j + 2]; }
    pthread_t th[64];
    bv_arg args[64];
    /* jobs split by output blocks, so the threads get equal work */
    int nt = 0;
    size_t j = 0;
    for (int i = 0; i < nthreads && j < njobs; i++) {
        size_t want = tot * (size_t)(i + 1) / (size_t)nthreads, j0 = j;
        while (j < njobs && (off[j] + jobs[3 * j + 2] <= want || j == j0)) j++;
        if (i == nthreads - 1) j = njobs;
        bv_arg a = { &src, packNum / (size_t)nchunks, packNum % (size_t)nchunks, bpp, jobs, start, has_start, off, out, j0, j };
        args[nt++] = a;
    }
    if (nt == 1) bv_worker(&args[0]);
    else {
        for (int i = 0; i < nt; i++) pthread_create(&th[i], NULL, bv_worker, &args[i]);
        for (int i = 0; i < nt; i++) pthread_join(th[i], NULL);
    }
    free(off);
    return 0;
}

/* ---- harness restatement (viterbiDF.h:20-167, main.cpp:131-137) ---- */

typedef struct { uint32_t mt[624]; int idx; } mt19937_t;
static void mt_seed(mt19937_t* m, uint32_t s)
{
    m->mt[0] = s;
    for (int i = 1; i < 624; i++) m->mt[i] = 1812433253u * (m->mt[i - 1] ^ (m->mt[i - 1] >> 30)) + (uint32_t)i;
    m->idx = 624;
}
static uint32_t mt_next(mt19937_t* m)
{
    if (m->idx >= 624) {
        for (int i = 0; i < 624; i++) {
            uint32_t y = (m->mt[i] & 0x80000000u) | (m->mt[(i + 1) % 624] & 0x7fffffffu);
            m->mt[i] = m->mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        m->idx = 0;
    }
    uint32_t y = m->mt[m->idx++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
}
/* generate_canonical<float,24>(mt19937) (libstdc++ 11 random.tcc:3348-3380) */
static float mt_canon_f(mt19937_t* m)
{
    float r = (float)mt_next(m) / 4294967296.0f;
    if (r >= 1.0f) r = nextafterf(1.0f, 0.0f);
    return r;
}
/* normal_distribution<float>, Marsaglia polar (random.tcc:1802-1834) */
typedef struct { int have; float saved; float stddev; } normal_t;
static float normal_draw(normal_t* n, mt19937_t* m)
{
    float ret;
    if (n->have) { n->have = 0; ret = n->saved; }
    else {
        float x, y, r2;
        do {
            x = (float)((double)(2.0f * mt_canon_f(m)) - 1.0);
            y = (float)((double)(2.0f * mt_canon_f(m)) - 1.0);
            r2 = x * x + y * y;
        } while (r2 > 1.0f || r2 == 0.0f);
        float mult = sqrtf(-2.0f * logf(r2) / r2);
        n->saved = x * mult;
        n->have = 1;
        ret = y * mult;
    }
    return ret * n->stddev + 0.0f;
}

/* restated generators exposed for the generator pin test */
void vo_gen_bits(uint32_t seed, size_t n, uint8_t* bits)
{
    mt19937_t m; mt_seed(&m, seed);
    for (size_t i = 0; i < n; i++) bits[i] = (uint8_t)(mt_next(&m) >> 31);
}
void vo_gen_normals(uint32_t seed, float stddev, size_t n, float* out)
{
    mt19937_t m; mt_seed(&m, seed);
    normal_t d = { 0, 0.0f, stddev };
    for (size_t i = 0; i < n; i++) out[i] = normal_draw(&d, &m);
}

/* raw std::mt19937(seed) outputs n0 .. n0+n-1 (for the jump-ahead tests) */
void vo_mt_raw(uint32_t seed, size_t n0, size_t n, uint32_t* out)
{
    mt19937_t m; mt_seed(&m, seed);
    for (size_t i = 0; i < n0; i++) (void)mt_next(&m);
    for (size_t i = 0; i < n; i++) out[i] = mt_next(&m);
}

/*
 * glibc 2.35 logf (x86-64 FMA variant, e_logf.c of the ARM optimized-routines, table __logf_data;
 * the variant glibc's ifunc selects on FMA/AVX2 hosts), restated with its table constants read from
 * this image's libm.  The GPU channel source (csrc/vd_mt.h glibc_logf) uses the same constants;
 * vo_logf_mismatch checks the restatement against the host logf.
 */
static const double vo_logf_tab[16][2] = {
    {0x1.661ec79f8f3bep+0, -0x1.57bf7808caadep-2}, {0x1.571ed4aaf883dp+0, -0x1.2bef0a7c06ddbp-2},
    {0x1.49539f0f010b0p+0, -0x1.01eae7f513a67p-2}, {0x1.3c995b0b80385p+0, -0x1.b31d8a68224e9p-3},
    {0x1.30d190c8864a5p+0, -0x1.6574f0ac07758p-3}, {0x1.25e227b0b8ea0p+0, -0x1.1aa2bc79c8100p-3},
    {0x1.1bb4a4a1a343fp+0, -0x1.a4e76ce8c0e5ep-4}, {0x1.12358f08ae5bap+0, -0x1.1973c5a611cccp-4},
    {0x1.0953f419900a7p+0, -0x1.252f438e10c1ep-5}, {0x1.0000000000000p+0, 0x0.0p+0},
    {0x1.e608cfd9a47acp-1, 0x1.aa5aa5df25984p-5}, {0x1.ca4b31f026aa0p-1, 0x1.c5e53aa362eb4p-4},
    {0x1.b2036576afce6p-1, 0x1.526e57720db08p-3}, {0x1.9c2d163a1aa2dp-1, 0x1.bc2860d224770p-3},
    {0x1.886e6037841edp-1, 0x1.1058bc8a07ee1p-2}, {0x1.767dcf5534862p-1, 0x1.4043057b6ee09p-2}};
float vo_logf_restated(float x)
{
    uint32_t ix; memcpy(&ix, &x, 4);
    if (ix == 0x3f800000u) return 0.0f;
    uint32_t tmp = ix - 0x3f330000u, iz = ix - (tmp & 0xff800000u);
    int i = (int)((tmp >> 19) & 15), k = (int32_t)tmp >> 23;
    float zf; memcpy(&zf, &iz, 4);
    double z = zf;
    double r = fma(z, vo_logf_tab[i][0], -1.0);
    double y0 = fma((double)k, 0x1.62e42fefa39efp-1, vo_logf_tab[i][1]);
    double y = fma(r, 0x1.5575b0be00b6ap-2, -0x1.ffffef20a4123p-2);
    double r2 = r * r;
    y = fma(r2, -0x1.00ea348b88334p-2, y);
    y = fma(r2, y, y0 + r);
    return (float)y;
}
/* floats with bit patterns lo, lo+stride, .. <= hi where vo_logf_restated differs from logf */
long long vo_logf_mismatch(uint32_t lo, uint32_t hi, uint32_t stride)
{
    long long bad = 0;
    for (uint64_t b = lo; b <= hi; b += stride) {
        uint32_t u = (uint32_t)b;
        float x; memcpy(&x, &u, 4);
        float a = logf(x), c = vo_logf_restated(x);
        if (memcmp(&a, &c, 4)) bad++;
    }
    return bad;
}

/* RandBitGen | ConvolutionalEncoder | AddNoise (viterbiDF.h:20-95): N bits, 2N float values */
void vo_channel(size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, int noiseless, uint8_t* bits,
                float* values)
{
    mt19937_t mb; mt_seed(&mb, bitSeed);
    for (size_t i = 0; i < N; i++) bits[i] = (uint8_t)(mt_next(&mb) >> 31);
    float stddev = (float)pow(10.0, (double)(-snr) / 5.0);
    mt19937_t mn; mt_seed(&mn, noiseSeed);
    normal_t nd = { 0, 0.0f, stddev };
    uint32_t buf = 0;
    for (size_t i = 0; i < N; i++) {
        buf >>= 1;
        buf |= (uint32_t)bits[i] << (CL - 1);
        int o[2] = { parity7((int)(buf & POLY0)), parity7((int)(buf & POLY1)) };
        for (int j = 0; j < 2; j++) {
            float base = o[j] ? 1.0f : -1.0f;
            values[2 * i + j] = noiseless ? base : base + normal_draw(&nd, &mn);
        }
    }
}

static inline uint32_t quant(int ch, float v)
{
    switch (ch) {
    case CH_HARD: return v > 0.0f ? 1u : 0u;
    case CH_SOFT4: { int q = (int)lrintf(v); if (q < -8) q = -8; if (q > 7) q = 7; return (uint32_t)q & 0xFu; }
    case CH_SOFT8: { int q = (int)lrintf(v); if (q < -128) q = -128; if (q > 127) q = 127; return (uint32_t)q & 0xFFu; }
    case CH_SOFT16: { long q = lrintf(v); if (q < -32768) q = -32768; if (q > 32767) q = 32767; return (uint32_t)q & 0xFFFFu; }
    }
    return 0;
}

/*
 * Reference pipeline RandBitGen(N,bitSeed) | ConvolutionalEncoder(7,0171,0133) |
 * AddNoise(10^(-snr/5), noiseSeed) | SoftDecisionPacker(inputType, 40000).
 * bits: N bytes (0/1).  packed: vo_input_size(opt, 2N) bytes.  N must be a multiple of 16.
 * noiseless != 0 reproduces the stddev = +inf branch (viterbiDF.h:79-85).
 */
int vo_simulate(int opt, size_t N, float snr, uint32_t bitSeed, uint32_t noiseSeed, int noiseless,
                uint8_t* bits, void* packed)
{
    int ch = CH(opt);
    if (N % 16) return -1;
    mt19937_t mb; mt_seed(&mb, bitSeed);
    for (size_t i = 0; i < N; i++) bits[i] = (uint8_t)(mt_next(&mb) >> 31);
    float stddev = (float)pow(10.0, (double)(-snr) / 5.0);
    mt19937_t mn; mt_seed(&mn, noiseSeed);
    normal_t nd = { 0, 0.0f, stddev };
    const float scale = 40000.0f;
    int packLen = 0, dpp = 0;
    switch (ch) {
    case CH_HARD: packLen = 1; dpp = 32; break;
    case CH_SOFT4: packLen = 4; dpp = 8; break;
    case CH_SOFT8: packLen = 8; dpp = 4; break;
    case CH_SOFT16: packLen = 16; dpp = 2; break;
    default: break;
    }
    uint32_t buf = 0, acc = 0;
    int nacc = 0;
    size_t wi = 0;
    uint32_t* pw = (uint32_t*)packed;
    float* pf = (float*)packed;
    for (size_t i = 0; i < N; i++) {
        buf >>= 1;
        buf |= (uint32_t)bits[i] << (CL - 1);
        int o[2] = { parity7((int)(buf & POLY0)), parity7((int)(buf & POLY1)) };
        for (int j = 0; j < 2; j++) {
            float base = o[j] ? 1.0f : -1.0f;
            float v = noiseless ? base : base + normal_draw(&nd, &mn);
            if (ch == CH_FP32) { pf[2 * i + j] = v * scale; continue; }
            acc = (acc << packLen) | quant(ch, v * scale);
            if (++nacc == dpp) { pw[wi++] = acc; acc = 0; nacc = 0; }
        }
    }
    return 0;
}

/*
 * SoftDecisionPacker::process (viterbiDF.h:98-167) on caller-given channel values: quantise v*scale
 * (quant(), viterbiDF.h:106-125 -- lrintf, then for SOFT4/SOFT8 the long is narrowed to int before
 * saturating, for SOFT16 saturated as a long) and pack dataPerPack codes MSB-first per 32-bit word;
 * FP32 writes v*scale (the reference returns src unchanged when scale == 1, identical values).
 * n values in, vo_input_size(opt, n) bytes out.  A trailing partial word (n not a multiple of
 * dataPerPack) packs the missing values as 0.0f; the reference reads past the end of its vector there.
 */
void vo_pack(int opt, const float* v, size_t n, float scale, void* packed)
{
    int ch = CH(opt);
    if (ch == CH_FP32) {
        float* pf = (float*)packed;
        for (size_t i = 0; i < n; i++) pf[i] = scale == 1.0f ? v[i] : v[i] * scale;
        return;
    }
    int packLen = 0, dpp = 0;
    switch (ch) {
    case CH_HARD: packLen = 1; dpp = 32; break;
    case CH_SOFT4: packLen = 4; dpp = 8; break;
    case CH_SOFT8: packLen = 8; dpp = 4; break;
    case CH_SOFT16: packLen = 16; dpp = 2; break;
    default: return;
    }
    uint32_t* pw = (uint32_t*)packed;
    for (size_t i = 0; i < n; i += (size_t)dpp) {
        uint32_t b = 0;
        for (size_t j = i; j < i + (size_t)dpp; j++) {
            float x = j < n ? v[j] : 0.0f;
            b = (b << packLen) | quant(ch, x * scale);
        }
        pw[i / (size_t)dpp] = b;
    }
}

/* BER count (main.cpp:151-171): decoded bit i vs source bit i + extraL */
long long vo_ben(int opt, const uint8_t* bits, size_t N, const void* dec, size_t decBytes)
{
    int bpp = bits_per_pack(opt);
    size_t nbits = decBytes * 8;
    long long ben = 0;
    for (size_t i = 0; i < nbits; i++) {
        int b;
        if (bpp == 32) b = (int)((((const uint32_t*)dec)[i / 32] >> (31 - i % 32)) & 1u);
        else b = (int)((((const uint16_t*)dec)[i / 16] >> (15 - i % 16)) & 1u);
        if (i + EXTRA_L >= N) { ben++; continue; }
        if (b != bits[i + EXTRA_L]) ben++;
    }
    return ben;
}
