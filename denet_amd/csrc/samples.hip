// GPU corner selection + RoI proposal: the MI355X counterpart of the reference's host C++
// `build_samples` (denet/layer/denet_sparse.cc:489-557 run_build_samples, :321-471 search_corners,
// :271-308 get_sample, :474-487 get_local_max), which the reference runs on CPU threads between two
// halves of the device step (denet/layer/denet_sparse.py:117-145).
//
// Pipeline (all on `stream`, no host round trip):
//   1. corner_select: one workgroup per (image, corner type). Threshold (+ optional local-max test)
//      over the log-probability plane in raster order; survivors are compacted with wave ballots and
//      a prefix sum over the wave counts, which preserves the reference's raster order. If more than
//      max_corners survive the list is bitonic-sorted in LDS by (logpr desc, raster asc) and truncated
//      (reference: std::partial_sort by logpr). Also emits a membership bitmap per corner type.
//   2. three histogram passes (12+12+8 bits) over the score keys of all TLxBR and TRxBL pairs: an exact
//      32-bit radix select of the sample_count-th best candidate. Pairs are enumerated on the fly; the
//      reference's unordered_map de-duplication reduces to an O(1) test (a TRxBL box is a duplicate
//      iff its TL and BR corners are both selected), because the two passes cannot repeat a box
//      internally.
//   3. collect + final bitonic sort by (key asc, generation index asc), emit integer boxes and |d|.
// Score key: pr = 1/(1+exp(|pr_f - pr_t|)) is strictly decreasing in |d|, so candidates are ranked by
// the fp32 bit pattern of |d| (ascending); the fp32 sums are evaluated in the reference's order, so
// the key is bit-identical to the reference's. The final pr is evaluated on the host by
// denet_samples_finish_host with the same libm expression as the reference (denet_sparse.cc:306).
// Compiled with -ffp-contract=off.
#include "common.h"
#include "../../include/denet_hip.h"
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

namespace {

constexpr int TIE_CAP = 4096;   // extra slots for candidates tying with the threshold key
// tie slots actually used: up to 7936 requested candidates the final sort keeps sample_count + ties <= 8192 candidates in LDS;
// beyond (RoI clustering of the 48 x 48 models asks for the 23 040 best, denet_sparse.cc:171-175) it sorts through a global
// buffer (pair_finalize_big_kernel) and the ties get their full 4096 slots
constexpr int SORT_LDS_MAX = 7936;
__host__ __device__ inline int tie_cap_for(int sample_count) {
    return (sample_count <= 4096 || sample_count > SORT_LDS_MAX) ? TIE_CAP : 8192 - sample_count;
}
constexpr int NBLK_PAIR = 64;   // workgroups per image for the pair passes

struct ImgState {
    unsigned prefix;   // key bits fixed so far
    unsigned need;     // how many more candidates are needed from the current bin
    unsigned done;     // 1: every candidate is selected (total <= sample_count)
    unsigned nless;    // collected candidates with key < T
    unsigned ntie;     // collected candidates with key == T
    unsigned total;    // number of candidates
    unsigned pad0, pad1;
};

__device__ __forceinline__ bool corner_before(float va, unsigned pa, float vb, unsigned pb) {
    return (va > vb) || (va == vb && pa < pb);
}

// max over [y-l, y+l) x [x-l, x+l) clipped to [0,H-1) x [0,W-1): upper bounds EXCLUSIVE and clipped to
// size-1 exactly as denet_sparse.cc:474-487
__device__ __forceinline__ float local_max_at(const float* plane, int H, int W, int y, int x, int l) {
    const int x0 = max(0, x - l), y0 = max(0, y - l);
    const int x1 = min(W - 1, x + l), y1 = min(H - 1, y + l);
    float m = -100000.f;
    for (int yy = y0; yy < y1; ++yy)
        for (int xx = x0; xx < x1; ++xx) m = fmaxf(m, plane[yy * W + xx]);
    return m;
}

__global__ __launch_bounds__(1024) void corner_select_kernel(const float* __restrict__ pr, int* __restrict__ corners,
                                                             int* __restrict__ ncorner, unsigned* __restrict__ bitmap,
                                                             int Cn, int H, int W, float thr, int max_corners,
                                                             int local_max, int NP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    float* sval = (float*)smem_raw;              // [NP]
    unsigned* spos = (unsigned*)(sval + NP);     // [NP]
    unsigned* sbits = spos + NP;                 // [HW/32 rounded up]
    __shared__ int sh_w[16];
    const int b = blockIdx.x, ci = blockIdx.y;
    const int HW = H * W;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* plane = pr + ((long)(b * 2 + 1) * Cn + ci) * HW;
    const int nwords = (HW + 31) / 32;
    for (int i = tid; i < nwords; i += 1024) sbits[i] = 0u;

    int base = 0;
    for (int chunk = 0; chunk < HW; chunk += 1024) {
        const int cell = chunk + tid;
        const bool valid = cell < HW;
        const float v = valid ? plane[cell] : 0.f;
        bool pred = valid && (v > thr);
        if (pred && local_max > 0) {
            const int y = cell / W, x = cell - y * W;
            if (v < local_max_at(plane, H, W, y, x, local_max)) pred = false;
        }
        const unsigned long long mask = __ballot(pred);
        const int wofs = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) sh_w[wave] = __popcll(mask);
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int c = sh_w[w];
            if (w < wave) wbase += c;
            total += c;
        }
        if (pred) {
            const int idx = base + wbase + wofs;
            sval[idx] = v;
            spos[idx] = (unsigned)cell;
        }
        base += total;
        __syncthreads();
    }
    int n = base;
    if (n > max_corners) {
        int np2 = 1;
        while (np2 < n) np2 <<= 1;
        for (int i = n + tid; i < np2; i += 1024) {
            sval[i] = -INFINITY;
            spos[i] = 0xFFFFFFFFu;
        }
        __syncthreads();
        for (int k = 2; k <= np2; k <<= 1) {
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int t = tid; t < np2 / 2; t += 1024) {
                    const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                    const int hi = lo | j;
                    const bool up = ((lo & k) == 0);
                    const float va = sval[lo], vb = sval[hi];
                    const unsigned pa = spos[lo], pb = spos[hi];
                    // ascending position in the "before" order: swap when hi should come before lo
                    const bool hi_first = corner_before(vb, pb, va, pa);
                    if (hi_first == up) {
                        sval[lo] = vb; sval[hi] = va;
                        spos[lo] = pb; spos[hi] = pa;
                    }
                }
                __syncthreads();
            }
        }
        n = max_corners;
    }
    int* cl = corners + ((long)b * Cn + ci) * max_corners;
    for (int i = tid; i < n; i += 1024) {
        const unsigned p = spos[i];
        cl[i] = (int)p;
        atomicOr(&sbits[p >> 5], 1u << (p & 31));
    }
    __syncthreads();
    unsigned* bm = bitmap + ((long)b * Cn + ci) * nwords;
    for (int i = tid; i < nwords; i += 1024) bm[i] = sbits[i];
    if (tid == 0) ncorner[b * Cn + ci] = n;
}

struct PairCtx {
    const float* pr;        // [B,2,Cn,H,W]
    const int* corners;     // [B,Cn,max_corners]
    const int* ncorner;     // [B,Cn]
    const unsigned* bitmap; // [B,Cn,nwords]
    int Cn, H, W, max_corners, nwords;
};

// enumerates the candidates of image b assigned to this thread and calls f(key, gen, x0, y0, x1, y1)
template <class F>
__device__ __forceinline__ void for_each_candidate(const PairCtx& c, int b, F&& f) {
    const int HW = c.H * c.W;
    const int* nc = c.ncorner + b * c.Cn;
    const int nTL = nc[0], nTR = nc[1], nBL = nc[2], nBR = nc[3];
    const int nC = (c.Cn == 5) ? nc[4] : 0;
    const int* cTL = c.corners + ((long)b * c.Cn + 0) * c.max_corners;
    const int* cTR = c.corners + ((long)b * c.Cn + 1) * c.max_corners;
    const int* cBL = c.corners + ((long)b * c.Cn + 2) * c.max_corners;
    const int* cBR = c.corners + ((long)b * c.Cn + 3) * c.max_corners;
    const int* cCC = c.corners + ((long)b * c.Cn + (c.Cn - 1)) * c.max_corners;     // centres (Cn == 5 only)
    const unsigned* bTL = c.bitmap + ((long)b * c.Cn + 0) * c.nwords;
    const unsigned* bTR = c.bitmap + ((long)b * c.Cn + 1) * c.nwords;
    const unsigned* bBL = c.bitmap + ((long)b * c.Cn + 2) * c.nwords;
    const unsigned* bBR = c.bitmap + ((long)b * c.Cn + 3) * c.nwords;
    auto has = [&](const unsigned* bm, int y, int x) { const int q = y * c.W + x; return ((bm[q >> 5] >> (q & 31)) & 1u) != 0u; };
    const float* pf = c.pr + (long)(b * 2 + 0) * c.Cn * HW;
    const float* pt = c.pr + (long)(b * 2 + 1) * c.Cn * HW;
    // generators in the reference's order (denet_sparse.cc:337-466): TLxBR, TRxBL, then centre x {TL, TR, BL, BR}.
    // A box has ONE centre, so boxes of different centres never coincide and a box generated from centre c by a later
    // corner type is a duplicate iff one of its earlier corner types is selected; all de-duplication is O(1) bitmap tests
    const unsigned P0 = (unsigned)nTL * (unsigned)nBR, P1 = (unsigned)nTR * (unsigned)nBL;
    const unsigned Q0 = (unsigned)nC * (unsigned)nTL, Q1 = (unsigned)nC * (unsigned)nTR, Q2 = (unsigned)nC * (unsigned)nBL,
                   Q3 = (unsigned)nC * (unsigned)nBR;
    const unsigned total = P0 + P1 + Q0 + Q1 + Q2 + Q3;
    for (unsigned p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        int x0, y0, x1, y1;
        if (p < P0) {
            const unsigned i = p / (unsigned)nBR, j = p - i * (unsigned)nBR;
            const int tl = cTL[i], br = cBR[j];
            y0 = tl / c.W; x0 = tl - y0 * c.W;
            y1 = br / c.W; x1 = br - y1 * c.W;
            if (x1 <= x0 || y1 <= y0) continue;
        } else if (p < P0 + P1) {
            const unsigned q = p - P0;
            const unsigned i = q / (unsigned)nBL, j = q - i * (unsigned)nBL;
            const int tr = cTR[i], bl = cBL[j];
            y0 = tr / c.W; x1 = tr - y0 * c.W;
            y1 = bl / c.W; x0 = bl - y1 * c.W;
            if (x1 <= x0 || y1 <= y0) continue;
            // already produced by the TLxBR pass?
            if (has(bTL, y0, x0) && has(bBR, y1, x1)) continue;
        } else {
            unsigned q = p - P0 - P1;
            int type = 0;
            if (q >= Q0) { q -= Q0; type = 1; if (q >= Q1) { q -= Q1; type = 2; if (q >= Q2) { q -= Q2; type = 3; } } }
            const unsigned nT = (type == 0) ? nTL : (type == 1) ? nTR : (type == 2) ? nBL : nBR;
            const int* cT = (type == 0) ? cTL : (type == 1) ? cTR : (type == 2) ? cBL : cBR;
            const unsigned i = q / nT, j = q - i * nT;       // centre i (outer), corner j (inner)
            const int cc = cCC[i], ct = cT[j];
            const int cy = cc / c.W, cx = cc - cy * c.W;
            const int ty = ct / c.W, tx = ct - ty * c.W;
            if (type == 0) { x0 = tx; y0 = ty; x1 = x0 + 2 * (cx - x0); y1 = y0 + 2 * (cy - y0); }
            else if (type == 1) { x1 = tx; y0 = ty; x0 = x1 - 2 * (x1 - cx); y1 = y0 + 2 * (cy - y0); }
            else if (type == 2) { x0 = tx; y1 = ty; x1 = x0 + 2 * (cx - x0); y0 = y1 - 2 * (y1 - cy); }
            else { x1 = tx; y1 = ty; x0 = x1 - 2 * (x1 - cx); y0 = y1 - 2 * (y1 - cy); }
            if (x0 < 0 || y0 < 0 || x1 >= c.W || y1 >= c.H || x1 <= x0 || y1 <= y0) continue;
            const bool tl = has(bTL, y0, x0), tr = has(bTR, y0, x1), bl = has(bBL, y1, x0), br = has(bBR, y1, x1);
            if ((tl && br) || (tr && bl)) continue;                       // produced by one of the corner-pair passes
            if ((type >= 1 && tl) || (type >= 2 && tr) || (type >= 3 && bl)) continue;   // earlier type, same centre
        }
        // denet_sparse.cc:276-303: sequential fp32 sums in the order TL, TR, BL, BR (, centre)
        float sf = 0.f, st = 0.f;
        sf += pf[0 * HW + y0 * c.W + x0];
        sf += pf[1 * HW + y0 * c.W + x1];
        sf += pf[2 * HW + y1 * c.W + x0];
        sf += pf[3 * HW + y1 * c.W + x1];
        st += pt[0 * HW + y0 * c.W + x0];
        st += pt[1 * HW + y0 * c.W + x1];
        st += pt[2 * HW + y1 * c.W + x0];
        st += pt[3 * HW + y1 * c.W + x1];
        if (c.Cn == 5) {
            const int mx = (x0 + x1) / 2, my = (y0 + y1) / 2;
            sf += pf[4 * HW + my * c.W + mx];
            st += pt[4 * HW + my * c.W + mx];
        }
        const unsigned key = __float_as_uint(fabsf(sf - st));
        f(key, p, x0, y0, x1, y1);
    }
}

// LEVEL 0: bin = key >> 20 ; LEVEL 1: (key>>20)==prefix>>20, bin = (key>>8)&0xFFF ; LEVEL 2: bin = key&0xFF
template <int LEVEL>
__global__ __launch_bounds__(256) void pair_hist_kernel(PairCtx c, const ImgState* __restrict__ state,
                                                        unsigned* __restrict__ hist) {
    __shared__ unsigned sh[4096];
    const int b = blockIdx.y;
    const ImgState st = state[b];
    if (LEVEL > 0 && st.done) return;
    for (int i = threadIdx.x; i < 4096; i += 256) sh[i] = 0u;
    __syncthreads();
    const unsigned prefix = st.prefix;
    for_each_candidate(c, b, [&](unsigned key, unsigned, int, int, int, int) {
        if (LEVEL == 0) {
            atomicAdd(&sh[key >> 20], 1u);
        } else if (LEVEL == 1) {
            if ((key >> 20) == (prefix >> 20)) atomicAdd(&sh[(key >> 8) & 0xFFFu], 1u);
        } else {
            if ((key >> 8) == (prefix >> 8)) atomicAdd(&sh[key & 0xFFu], 1u);
        }
    });
    __syncthreads();
    unsigned* h = hist + (long)b * 4096;
    for (int i = threadIdx.x; i < 4096; i += 256)
        if (sh[i]) atomicAdd(&h[i], sh[i]);
}

// one workgroup per image: parallel scan of the histogram (256 threads x 16 bins)
template <int LEVEL>
__global__ __launch_bounds__(256) void pair_pick_kernel(ImgState* __restrict__ state, unsigned* __restrict__ hist,
                                                        int sample_count, int B) {
    __shared__ unsigned ssum[256];
    __shared__ unsigned s_sel, s_cum;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    unsigned* h = hist + (long)b * 4096;
    constexpr int NB = (LEVEL == 2) ? 256 : 4096;
    constexpr int PER = NB / 256;
    unsigned loc[PER];
    unsigned mine = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        loc[i] = h[tid * PER + i];
        mine += loc[i];
        h[tid * PER + i] = 0u;          // ready for the next level
    }
    ssum[tid] = mine;
    if (tid == 0) { s_sel = NB - 1; s_cum = 0xFFFFFFFFu; }
    __syncthreads();
    // inclusive scan over the 256 per-thread sums
    for (int o = 1; o < 256; o <<= 1) {
        const unsigned v = (tid >= o) ? ssum[tid - o] : 0u;
        __syncthreads();
        ssum[tid] += v;
        __syncthreads();
    }
    ImgState st = state[b];
    const unsigned total = ssum[255];
    if (LEVEL == 0) {
        st.total = total;
        st.need = (unsigned)sample_count;
        st.prefix = 0;
        st.done = (total <= (unsigned)sample_count) ? 1u : 0u;
        if (st.done) st.prefix = 0xFFFFFFFFu;
    }
    if (!st.done) {
        // the first bin whose inclusive cumulative count reaches `need`
        const unsigned before = ssum[tid] - mine;
        if (before < st.need && ssum[tid] >= st.need) {
            unsigned cum = before;
            for (int i = 0; i < PER; ++i) {
                if (cum + loc[i] >= st.need) {
                    s_sel = tid * PER + i;
                    s_cum = cum;
                    break;
                }
                cum += loc[i];
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        if (!st.done) {
            const unsigned sel = s_sel;
            const unsigned cum = (s_cum == 0xFFFFFFFFu) ? 0u : s_cum;   // unreachable: need <= total at every level
            st.need -= cum;
            if (LEVEL == 0) st.prefix = sel << 20;
            else if (LEVEL == 1) st.prefix |= sel << 8;
            else st.prefix |= sel;
        }
        state[b] = st;
    }
}

struct Cand {
    unsigned key, gen, box;   // box = x0 | y0<<8 | x1<<16 | y1<<24
};

__global__ __launch_bounds__(256) void pair_collect_kernel(PairCtx c, ImgState* __restrict__ state,
                                                           Cand* __restrict__ cand, int sample_count) {
    const int b = blockIdx.y;
    const unsigned T = state[b].prefix;
    const bool all = state[b].done != 0;
    Cand* out = cand + (long)b * (sample_count + TIE_CAP);
    for_each_candidate(c, b, [&](unsigned key, unsigned gen, int x0, int y0, int x1, int y1) {
        Cand e;
        e.key = key;
        e.gen = gen;
        e.box = (unsigned)x0 | ((unsigned)y0 << 8) | ((unsigned)x1 << 16) | ((unsigned)y1 << 24);
        if (all || key < T) {
            const unsigned slot = atomicAdd(&state[b].nless, 1u);
            if (slot < (unsigned)sample_count) out[slot] = e;
        } else if (key == T) {
            const unsigned slot = atomicAdd(&state[b].ntie, 1u);
            if (slot < (unsigned)tie_cap_for(sample_count)) out[sample_count + slot] = e;
        }
    });
}

__device__ __forceinline__ bool cand_before(const Cand& a, const Cand& b) {
    return (a.key < b.key) || (a.key == b.key && a.gen < b.gen);
}

// sorts the collected candidates by (key, gen) and writes the first sample_count
__global__ __launch_bounds__(1024) void pair_finalize_kernel(const ImgState* __restrict__ state,
                                                             const Cand* __restrict__ cand, int sample_count,
                                                             int* __restrict__ out_box, float* __restrict__ out_absd,
                                                             int* __restrict__ out_count, int NP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Cand* s = (Cand*)smem_raw;  // [NP]
    const int b = blockIdx.x;
    const ImgState st = state[b];
    const int nless = min((int)st.nless, sample_count);
    const int ntie = min((int)st.ntie, tie_cap_for(sample_count));
    const Cand* in = cand + (long)b * (sample_count + TIE_CAP);
    const int n = nless + ntie;
    // the network sorts the smallest power of two that holds the n candidates there are (a cold corner detector proposes none:
    // nothing to sort, 5 us instead of 100), padded with keys that sort last
    int np = 1;
    while (np < n) np <<= 1;
    if (np > NP) np = NP;
    for (int i = threadIdx.x; i < np; i += 1024) {
        Cand e;
        if (i < nless) e = in[i];
        else if (i < n) e = in[sample_count + (i - nless)];
        else { e.key = 0xFFFFFFFFu; e.gen = 0xFFFFFFFFu; e.box = 0; }
        s[i] = e;
    }
    __syncthreads();
    for (int k = 2; k <= np; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < np / 2; t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool up = ((lo & k) == 0);
                const Cand a = s[lo], c2 = s[hi];
                if (cand_before(c2, a) == up) {
                    s[lo] = c2;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
    }
    const int nout = min(n, sample_count);
    for (int i = threadIdx.x; i < sample_count; i += 1024) {
        int* ob = out_box + ((long)b * sample_count + i) * 4;
        if (i < nout) {
            const Cand e = s[i];
            ob[0] = e.box & 0xFF; ob[1] = (e.box >> 8) & 0xFF; ob[2] = (e.box >> 16) & 0xFF; ob[3] = (e.box >> 24) & 0xFF;
            out_absd[(long)b * sample_count + i] = __uint_as_float(e.key);
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0;
            out_absd[(long)b * sample_count + i] = 0.f;
        }
    }
    if (threadIdx.x == 0) out_count[b] = nout;
}

// The same for more candidates than LDS holds (sample_count > 7936): bitonic network over a global buffer of np (a power of
// two) candidates per image, one workgroup per image. Compare-exchange distances below 8192 run inside LDS on chunks of 8192
// candidates, the longer ones (the first steps of the last merge stages) through global memory - the buffer of an image is a few
// hundred KB and stays in L2. Same order as the single-pass kernel: (key, generation index) ascending.
constexpr int BIG_CHUNK = 8192;
__global__ __launch_bounds__(1024) void pair_finalize_big_kernel(const ImgState* __restrict__ state, const Cand* __restrict__ cand,
                                                                 Cand* __restrict__ sortbuf, int sample_count, int* __restrict__ out_box,
                                                                 float* __restrict__ out_absd, int* __restrict__ out_count, int NP) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    Cand* s = (Cand*)smem_raw;  // [BIG_CHUNK]
    const int b = blockIdx.x;
    const ImgState st = state[b];
    const int nless = min((int)st.nless, sample_count);
    const int ntie = min((int)st.ntie, tie_cap_for(sample_count));
    const Cand* in = cand + (long)b * (sample_count + TIE_CAP);
    Cand* g = sortbuf + (long)b * NP;
    const int n = nless + ntie;
    int np = BIG_CHUNK;
    while (np < n) np <<= 1;
    if (np > NP) np = NP;
    for (int i = threadIdx.x; i < np; i += 1024) {
        Cand e;
        if (i < nless) e = in[i];
        else if (i < n) e = in[sample_count + (i - nless)];
        else { e.key = 0xFFFFFFFFu; e.gen = 0xFFFFFFFFu; e.box = 0; }
        g[i] = e;
    }
    __syncthreads();
    // steps (k, j) of the network on chunk c in LDS, for j from jtop down to 1; `up` comes from the GLOBAL index
    auto lds_steps = [&](int c, int k, int jtop) {
        for (int i = threadIdx.x; i < BIG_CHUNK; i += 1024) s[i] = g[c * BIG_CHUNK + i];
        __syncthreads();
        for (int j = jtop; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < BIG_CHUNK / 2; t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool up = (((c * BIG_CHUNK + lo) & k) == 0);
                const Cand a = s[lo], c2 = s[hi];
                if (cand_before(c2, a) == up) {
                    s[lo] = c2;
                    s[hi] = a;
                }
            }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < BIG_CHUNK; i += 1024) g[c * BIG_CHUNK + i] = s[i];
        __syncthreads();
    };
    const int chunks = np / BIG_CHUNK;
    for (int c = 0; c < chunks; ++c)
        for (int k = 2; k <= BIG_CHUNK; k <<= 1) {
            // (a chunk is loaded and stored once per k here: 13 round trips of 96 KB through L2 per chunk, a few microseconds)
            lds_steps(c, k, k >> 1);
        }
    for (int k = 2 * BIG_CHUNK; k <= np; k <<= 1) {
        for (int j = k >> 1; j >= BIG_CHUNK; j >>= 1) {
            for (int t = threadIdx.x; t < np / 2; t += 1024) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int hi = lo | j;
                const bool up = ((lo & k) == 0);
                const Cand a = g[lo], c2 = g[hi];
                if (cand_before(c2, a) == up) {
                    g[lo] = c2;
                    g[hi] = a;
                }
            }
            __syncthreads();       // one workgroup owns the image's buffer: its own global writes are visible to it after the barrier
        }
        for (int c = 0; c < chunks; ++c) lds_steps(c, k, BIG_CHUNK >> 1);
    }
    const int nout = min(n, sample_count);
    for (int i = threadIdx.x; i < sample_count; i += 1024) {
        int* ob = out_box + ((long)b * sample_count + i) * 4;
        if (i < nout) {
            const Cand e = g[i];
            ob[0] = e.box & 0xFF; ob[1] = (e.box >> 8) & 0xFF; ob[2] = (e.box >> 16) & 0xFF; ob[3] = (e.box >> 24) & 0xFF;
            out_absd[(long)b * sample_count + i] = __uint_as_float(e.key);
        } else {
            ob[0] = ob[1] = ob[2] = ob[3] = 0;
            out_absd[(long)b * sample_count + i] = 0.f;
        }
    }
    if (threadIdx.x == 0) out_count[b] = nout;
}

struct WsLayout {
    size_t corners, ncorner, bitmap, hist, state, cand, sortbuf, total;
    int nwords;
};

WsLayout ws_layout(int B, int Cn, int H, int W, int max_corners, int sample_count) {
    WsLayout l;
    l.nwords = (H * W + 31) / 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    l.corners = take((size_t)B * Cn * max_corners * sizeof(int));
    l.ncorner = take((size_t)B * Cn * sizeof(int));
    l.bitmap = take((size_t)B * Cn * l.nwords * sizeof(unsigned));
    l.hist = take((size_t)B * 4096 * sizeof(unsigned));
    l.state = take((size_t)B * sizeof(ImgState));
    l.cand = take((size_t)B * (sample_count + TIE_CAP) * sizeof(Cand));
    l.sortbuf = o;
    if (sample_count > SORT_LDS_MAX) {       // the global sort buffer of pair_finalize_big_kernel
        size_t np = BIG_CHUNK;
        while (np < (size_t)sample_count + TIE_CAP) np <<= 1;
        l.sortbuf = take((size_t)B * np * sizeof(Cand));
    }
    l.total = o;
    return l;
}

}  // namespace

extern "C" size_t denet_build_samples_workspace_bytes(int B, int Cn, int H, int W, int max_corners, int sample_count) {
    if (B <= 0 || Cn <= 0 || H <= 0 || W <= 0 || max_corners <= 0 || sample_count <= 0) return 0;
    return ws_layout(B, Cn, H, W, max_corners, sample_count).total;
}

extern "C" int denet_build_samples(const float* corner_pr, int* out_box, float* out_absd, int* out_count,
                                   void* workspace, size_t workspace_bytes, int B, int Cn, int H, int W,
                                   float corner_threshold, int sample_count, int max_corners, int local_max,
                                   hipStream_t stream) {
    DENET_CHECK_ARG(corner_pr && out_box && out_absd && out_count && workspace, "build_samples: null pointer");
    DENET_CHECK_ARG(Cn == 4 || Cn == 5, "build_samples: Cn must be 4 or 5 (corner types + optional centre), got %d", Cn);
    DENET_CHECK_ARG(H > 0 && W > 0 && H <= 256 && W <= 256 && H * W <= 16384, "build_samples: map %dx%d unsupported", H, W);
    DENET_CHECK_ARG(max_corners > 0 && max_corners <= 1024, "build_samples: max_corners must be in 1..1024");
    // the final per-image sort holds sample_count + tie slots in LDS (<= 8192 candidates, 96 KB) or, beyond 7936 requested
    // candidates, sorts through a global buffer; 61 440 = ten times the 78 x 78 RoIs of the largest model the reference describes
    DENET_CHECK_ARG(sample_count > 0 && sample_count <= 61440, "build_samples: sample_count must be in 1..61440");
    DENET_CHECK_ARG(local_max >= 0, "build_samples: negative local_max");
    const WsLayout l = ws_layout(B, Cn, H, W, max_corners, sample_count);
    DENET_CHECK_ARG(workspace_bytes >= l.total, "build_samples: workspace too small (%zu < %zu)", workspace_bytes, l.total);
    char* ws = (char*)workspace;
    int* corners = (int*)(ws + l.corners);
    int* ncorner = (int*)(ws + l.ncorner);
    unsigned* bitmap = (unsigned*)(ws + l.bitmap);
    unsigned* hist = (unsigned*)(ws + l.hist);
    ImgState* state = (ImgState*)(ws + l.state);
    Cand* cand = (Cand*)(ws + l.cand);
    // denet_sparse.cc:503: float threshold = std::log(corner_threshold)
    const float thr = logf(corner_threshold);

    hipError_t e = hipMemsetAsync(ws + l.hist, 0, l.cand - l.hist, stream);   // hist + state
    if (e != hipSuccess) {
        denet_set_error("build_samples: hipMemsetAsync: %s", hipGetErrorString(e));
        return -(int)e;
    }
    int NP = 1;
    while (NP < H * W) NP <<= 1;
    const size_t lds1 = (size_t)NP * 8 + (size_t)l.nwords * 4;
    static size_t lds1_set = 0, lds2_set = 0;
    if (lds1 > lds1_set) {
        e = hipFuncSetAttribute((const void*)corner_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds1);
        if (e != hipSuccess) { denet_set_error("build_samples: LDS attr: %s", hipGetErrorString(e)); return -(int)e; }
        lds1_set = lds1;
    }
    hipLaunchKernelGGL(corner_select_kernel, dim3(B, Cn), dim3(1024), lds1, stream, corner_pr, corners, ncorner, bitmap,
                       Cn, H, W, thr, max_corners, local_max, NP);
    PairCtx c;
    c.pr = corner_pr; c.corners = corners; c.ncorner = ncorner; c.bitmap = bitmap;
    c.Cn = Cn; c.H = H; c.W = W; c.max_corners = max_corners; c.nwords = l.nwords;
    const dim3 pg(NBLK_PAIR, B), pickg(B);
    hipLaunchKernelGGL(pair_hist_kernel<0>, pg, dim3(256), 0, stream, c, state, hist);
    hipLaunchKernelGGL(pair_pick_kernel<0>, pickg, dim3(256), 0, stream, state, hist, sample_count, B);
    hipLaunchKernelGGL(pair_hist_kernel<1>, pg, dim3(256), 0, stream, c, state, hist);
    hipLaunchKernelGGL(pair_pick_kernel<1>, pickg, dim3(256), 0, stream, state, hist, sample_count, B);
    hipLaunchKernelGGL(pair_hist_kernel<2>, pg, dim3(256), 0, stream, c, state, hist);
    hipLaunchKernelGGL(pair_pick_kernel<2>, pickg, dim3(256), 0, stream, state, hist, sample_count, B);
    hipLaunchKernelGGL(pair_collect_kernel, pg, dim3(256), 0, stream, c, state, cand, sample_count);
    int NP2 = 1;
    while (NP2 < sample_count + tie_cap_for(sample_count)) NP2 <<= 1;
    const bool big = sample_count > SORT_LDS_MAX;
    const size_t lds2 = (size_t)(big ? BIG_CHUNK : NP2) * sizeof(Cand);
    static size_t lds3_set = 0;
    size_t& set = big ? lds3_set : lds2_set;
    if (lds2 > set) {
        e = hipFuncSetAttribute(big ? (const void*)pair_finalize_big_kernel : (const void*)pair_finalize_kernel,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2);
        if (e != hipSuccess) { denet_set_error("build_samples: LDS attr: %s", hipGetErrorString(e)); return -(int)e; }
        set = lds2;
    }
    if (big) {
        if (NP2 < BIG_CHUNK) NP2 = BIG_CHUNK;
        hipLaunchKernelGGL(pair_finalize_big_kernel, dim3(B), dim3(1024), lds2, stream, state, cand, (Cand*)(ws + l.sortbuf), sample_count,
                           out_box, out_absd, out_count, NP2);
    } else {
        hipLaunchKernelGGL(pair_finalize_kernel, dim3(B), dim3(1024), lds2, stream, state, cand, sample_count, out_box,
                           out_absd, out_count, NP2);
    }
    DENET_CHECK_LAUNCH("build_samples");
    return DENET_OK;
}

// Diagnostic read-out of the LAST denet_build_samples call on this workspace (same geometry arguments): corners kept per
// (image, type) after the max_corners truncation (denet_sparse.cc:526-530) and candidate boxes generated per image by the
// pair search (:337-373, before the top-sample_count cut). Device-to-device copies on `stream`; ncorner_out [B*Cn] int32,
// candidates_out [B] uint32 (device).
extern "C" int denet_build_samples_stats(const void* workspace, size_t workspace_bytes, int B, int Cn, int H, int W,
                                         int max_corners, int sample_count, int* ncorner_out, unsigned* candidates_out,
                                         hipStream_t stream) {
    DENET_CHECK_ARG(workspace && ncorner_out && candidates_out, "build_samples_stats: null pointer");
    DENET_CHECK_ARG(B > 0 && (Cn == 4 || Cn == 5) && H > 0 && W > 0 && max_corners > 0 && sample_count > 0,
                    "build_samples_stats: bad geometry");
    const WsLayout l = ws_layout(B, Cn, H, W, max_corners, sample_count);
    DENET_CHECK_ARG(workspace_bytes >= l.total, "build_samples_stats: workspace too small");
    const char* ws = (const char*)workspace;
    hipError_t e = hipMemcpyAsync(ncorner_out, ws + l.ncorner, (size_t)B * Cn * sizeof(int), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess)
        e = hipMemcpy2DAsync(candidates_out, sizeof(unsigned), ws + l.state + offsetof(ImgState, total), sizeof(ImgState),
                             sizeof(unsigned), (size_t)B, hipMemcpyDeviceToDevice, stream);
    if (e != hipSuccess) {
        denet_set_error("build_samples_stats: copy: %s", hipGetErrorString(e));
        return -(int)e;
    }
    return DENET_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The training-time RoI list editing (denet/layer/denet_sparse.py:184-201) ON THE DEVICE, for the batches that need no
// random.sample: every image proposes at most n_keep RoIs (a detector early in training; the host checks the counts). Then the
// edited list of image b is: its count[b] proposals, (S - count[b]) random boxes, the last n_gt of them replaced by the ground
// truth - and the generator outputs a random box draws sit at a position that follows from the counts alone: 8 outputs per
// box (four `random()` of two outputs each, in the order x0, y0, x1, y1), images in order. The outputs come from a stretch drawn
// ahead on the host (denet_host_mt_prefetch) and uploaded at the start of the step; the host walks through the same stretch
// later, off the critical path, for the Python-side list (denet_host_edit_samples_stream) - same values, bit for bit:
//   proposal  -> denet_samples_finish_host's box arithmetic, (float)((double)x0 / W) ...
//   random    -> x0 = 0.0 + (1.0 - 0.0) * r, x1 = x0 + (1.0 - x0) * r (random.uniform), r = (a >> 5) * 2^26 + (b >> 6)) / 2^53,
//                doubles, no contraction (this file is compiled with -ffp-contract=off), rounded to fp32 on store
//   truth     -> (float)gt
// One workgroup per image, a thread per RoI slot. out_bbox [B][S][4] floats = what build_bbox_array would upload.
static __global__ __launch_bounds__(256) void edit_samples_kernel(const int* __restrict__ box, const int* __restrict__ count, int H, int W,
                                                           const uint32_t* __restrict__ mt_out, long n_out, long cursor0,
                                                           const double* __restrict__ gt, const int* __restrict__ gt_off,
                                                           int sample_gt, int S, int n_keep, float* __restrict__ out_bbox,
                                                           int* __restrict__ status) {
    const int b = blockIdx.x;
    long first = cursor0;                    // outputs drawn by the images before this one
    bool bad = false;
    for (int i = 0; i < b; ++i) {
        const int c = count[i];
        bad |= c > n_keep;
        first += 8L * (S - (c < S ? c : S));
    }
    const int n = count[b];
    bad |= n > n_keep || n < 0 || first + 8L * (S - n) > n_out;
    if (bad) {                               // not this kernel's case (or the stretch is too short): the host must not use the result
        if (threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const int g0 = sample_gt ? gt_off[b] : 0, ng = sample_gt ? gt_off[b + 1] - g0 : 0;
    for (int i = threadIdx.x; i < S; i += blockDim.x) {
        float* o = out_bbox + ((long)b * S + i) * 4;
        if (i >= S - ng) {
            const double* g = gt + (long)(g0 + (S - 1 - i)) * 4;
            o[0] = (float)g[0]; o[1] = (float)g[1]; o[2] = (float)g[2]; o[3] = (float)g[3];
        } else if (i < n) {
            const int* bx = box + ((long)b * S + i) * 4;
            // through fp32 and back, as the host list holds the fp32 tuple of denet_samples_finish_host
            o[0] = (float)((double)bx[0] / W);
            o[1] = (float)((double)bx[1] / H);
            o[2] = (float)((double)(bx[2] + 1) / W);
            o[3] = (float)((double)(bx[3] + 1) / H);
        } else {
            const uint32_t* m = mt_out + first + 8L * (i - n);
            double r[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const uint32_t a = m[2 * k] >> 5, c2 = m[2 * k + 1] >> 6;
                r[k] = (a * 67108864.0 + c2) * (1.0 / 9007199254740992.0);
            }
            const double x0 = 0.0 + (1.0 - 0.0) * r[0];
            const double y0 = 0.0 + (1.0 - 0.0) * r[1];
            const double x1 = x0 + (1.0 - x0) * r[2];
            const double y1 = y0 + (1.0 - y0) * r[3];
            o[0] = (float)x0; o[1] = (float)y0; o[2] = (float)x1; o[3] = (float)y1;
        }
    }
    if (b == (int)gridDim.x - 1 && threadIdx.x == 0) {
        const long used = first + 8L * (S - n) - cursor0;
        status[1] = (int)used;               // outputs consumed by the batch (the host arrives at the same number)
    }
}

// box [B][S][4] int32 and count [B]: denet_build_samples' outputs as they lie on the device; H, W: the corner map; mt_out [n_out]:
// the generator outputs drawn ahead, cursor0 = how many of them earlier draws of the step have used; gt [n][4] doubles + gt_off
// [B + 1] (sample_gt != 0); status [2] int32, zeroed here: [0] != 0 afterwards = an image proposed more than n_keep RoIs or the
// stretch is too short - out_bbox is then incomplete and the caller edits on the host as before; [1] = outputs consumed.
extern "C" int denet_edit_samples_device(const int* box, const int* count, int H, int W, const uint32_t* mt_out, long n_out,
                                         long cursor0, const double* gt, const int* gt_off, int sample_gt, int B, int S, int n_keep,
                                         float* out_bbox, int* status, hipStream_t stream) {
    DENET_CHECK_ARG(box && count && mt_out && out_bbox && status, "edit_samples_device: null pointer");
    DENET_CHECK_ARG(!sample_gt || (gt && gt_off), "edit_samples_device: ground truth missing");
    DENET_CHECK_ARG(B > 0 && S > 0 && n_keep >= 0 && n_keep <= S && H > 0 && W > 0 && n_out >= 0 && cursor0 >= 0,
                    "edit_samples_device: bad sizes");
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int), stream);
    if (e != hipSuccess) {
        denet_set_error("edit_samples_device: memset: %s", hipGetErrorString(e));
        return -(int)e;
    }
    hipLaunchKernelGGL(edit_samples_kernel, dim3(B), dim3(256), 0, stream, box, count, H, W, mt_out, n_out, cursor0, gt, gt_off,
                       sample_gt, S, n_keep, out_bbox, status);
    DENET_CHECK_LAUNCH("edit_samples_device");
    return DENET_OK;
}

// Host epilogue: turns the integer boxes + |d| of denet_build_samples (copied to the host) into the
// reference's sample tuples (pr, x0, y0, x1, y1) with the reference's exact host arithmetic
// (denet_sparse.cc:306-307): pr = (float)(1.0 / (1.0 + std::exp(fabs(d)))) with the fp32 exp overload,
// box = ((double)x0/W, (double)y0/H, (double)(x1+1)/W, (double)(y1+1)/H) rounded to fp32.
extern "C" int denet_samples_finish_host(const int* box_host, const float* absd_host, const int* count_host, int B,
                                         int sample_count, int H, int W, float* samples_host) {
    DENET_CHECK_ARG(box_host && absd_host && count_host && samples_host, "samples_finish_host: null pointer");
    for (int b = 0; b < B; ++b) {
        for (int i = 0; i < sample_count; ++i) {
            float* s = samples_host + ((long)b * sample_count + i) * 5;
            if (i < count_host[b]) {
                const int* bx = box_host + ((long)b * sample_count + i) * 4;
                const float d = absd_host[(long)b * sample_count + i];
                s[0] = (float)(1.0 / (1.0 + (double)expf(d)));
                s[1] = (float)((double)bx[0] / W);
                s[2] = (float)((double)bx[1] / H);
                s[3] = (float)((double)(bx[2] + 1) / W);
                s[4] = (float)((double)(bx[3] + 1) / H);
            } else {
                s[0] = s[1] = s[2] = s[3] = s[4] = 0.f;
            }
        }
    }
    return DENET_OK;
}

// apply_cluster of the RoI proposal (denet/layer/denet_sparse.cc:165-242; enabled when the DNS layer's nmsThreshold < 1
// and an image has more than sample_num^2 candidates, :541-542). Host code like the reference's: the device hands over the
// 10 * sample_num^2 best candidates in rank order (the clustering input, :171-175) and this routine groups them.
//   A candidate joins every group that holds a member with IoU > threshold (fp32 IoU, bounding-box reject first); it is
//   appended to the LAST such group in creation order and the other hit groups are merged into that one. If more than
//   output_num groups remain, the largest are kept (stable by creation order). Each group contributes its
//   1 + floor(size * ratio) best members, ratio = (output_num - groups) / (n - groups) in double; the result is ranked and
//   cut to output_num (:547-549).
// samples_host: [n][5] = pr, x0, y0, x1, y1 in rank order; out_host: [output_num][5]; out_count: rows written.
namespace {
struct CSample { float v[5]; };
inline float cs_overlap(const float* a, const float* b) {
    const float dx = fmaxf(0.0f, fminf(a[3], b[3]) - fmaxf(a[1], b[1]));
    const float dy = fmaxf(0.0f, fminf(a[4], b[4]) - fmaxf(a[2], b[2]));
    return dx * dy;
}
inline float cs_area(const float* a) { return (a[3] - a[1]) * (a[4] - a[2]); }
struct CGroup {
    float box[5];
    std::vector<int> head;                    // members appended one by one
    std::vector<std::vector<int>> merged;     // member lists of the groups merged into this one, in merge order
    bool alive = true;
    size_t size() const {
        size_t n = head.size();
        for (const auto& m : merged) n += m.size();
        return n;
    }
};
}  // namespace

extern "C" int denet_host_cluster_samples(const float* samples_host, int n, float threshold, int output_num, float* out_host,
                                          int* out_count) {
    DENET_CHECK_ARG(samples_host && out_host && out_count, "cluster_samples: null pointer");
    DENET_CHECK_ARG(n > output_num && output_num > 0, "cluster_samples: needs more candidates (%d) than outputs (%d)", n, output_num);
    std::vector<CGroup> groups;          // creation order; dead entries stay in place
    auto grow = [](float* box, const float* s) {
        box[0] = fmaxf(s[0], box[0]);
        box[1] = fminf(s[1], box[1]);
        box[2] = fminf(s[2], box[2]);
        box[3] = fmaxf(s[3], box[3]);
        box[4] = fmaxf(s[4], box[4]);
    };
    std::vector<int> hit;
    for (int i = 0; i < n; ++i) {
        const float* s = samples_host + 5 * (size_t)i;
        const float sa = cs_area(s);
        hit.clear();
        for (size_t g = 0; g < groups.size(); ++g) {
            const CGroup& G = groups[g];
            if (!G.alive || cs_overlap(s, G.box) == 0) continue;
            bool found = false;
            auto test = [&](const std::vector<int>& members) {
                for (int m : members) {
                    const float* t = samples_host + 5 * (size_t)m;
                    const float ai = cs_overlap(s, t);
                    const float au = sa + cs_area(t) - ai;
                    if (ai / au > threshold) return true;
                }
                return false;
            };
            found = test(G.head);
            for (size_t k = 0; !found && k < G.merged.size(); ++k) found = test(G.merged[k]);
            if (found) hit.push_back((int)g);
        }
        if (hit.empty()) {
            CGroup G;
            memcpy(G.box, s, sizeof(G.box));
            G.head.push_back(i);
            groups.push_back(std::move(G));
        } else {
            CGroup& T = groups[hit.back()];
            T.head.push_back(i);
            grow(T.box, s);
            for (size_t h = 0; h + 1 < hit.size(); ++h) {
                CGroup& O = groups[hit[h]];
                grow(T.box, O.box);
                T.merged.push_back(std::move(O.head));
                for (auto& m : O.merged) T.merged.push_back(std::move(m));
                O.merged.clear();
                O.alive = false;
            }
        }
    }
    std::vector<int> order;
    for (size_t g = 0; g < groups.size(); ++g)
        if (groups[g].alive) order.push_back((int)g);
    if ((int)order.size() > output_num) {
        std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return groups[a].size() > groups[b].size(); });
        order.resize(output_num);
    }
    const double ratio = (double)(output_num - (int)order.size()) / (double)(n - (int)order.size());
    std::vector<int> picked, all;
    auto better = [&](int a, int b) { return samples_host[5 * (size_t)a] > samples_host[5 * (size_t)b]; };
    for (int g : order) {
        const CGroup& G = groups[g];
        all.assign(G.head.begin(), G.head.end());
        for (const auto& m : G.merged) all.insert(all.end(), m.begin(), m.end());
        const size_t take = 1 + (size_t)floor((double)all.size() * ratio);
        std::stable_sort(all.begin(), all.end(), better);      // ties: member order (the reference's is unspecified)
        picked.insert(picked.end(), all.begin(), all.begin() + take);
    }
    std::stable_sort(picked.begin(), picked.end(), better);
    const int nout = std::min((int)picked.size(), output_num);
    for (int i = 0; i < nout; ++i) memcpy(out_host + 5 * (size_t)i, samples_host + 5 * (size_t)picked[i], 5 * sizeof(float));
    *out_count = nout;
    return DENET_OK;
}
