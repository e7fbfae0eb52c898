// RoI clustering ON THE DEVICE (opt-in, ops.CLUSTER_DEVICE): the counterpart of denet_host_cluster_samples (csrc/samples.hip),
// i.e. of the reference's apply_cluster (denet/layer/denet_sparse.cc:165-242) + the final ranking (:547-549), for thresholds in
// [0, 1). Input and output are in denet_build_samples' format (integer boxes, |d|, counts), so everything behind the call sees an
// ordinary sample_num^2 proposal.
//
// apply_cluster visits the n ranked candidates in order; a candidate joins every cluster holding a member with IoU > threshold and
// the hit clusters merge into the LAST of them in list order. For 0 <= threshold < 1 this has a closed form ("RoI
// clustering on the device"):
//   1. the final clusters are the connected components of the graph with an edge i - j wherever fp32 overlap_iou(i, j) > threshold
//      (the bounding-box reject of ClusterType::overlap never removes an edge: no overlap with the union box = IoU 0 with every
//      member);
//   2. candidate i creates a cluster iff it has no edge to a j < i; a merge keeps the last hit cluster, so a component stands in the
//      reference's list where its YOUNGEST creator stood: key = max{i in component : no edge to a smaller index};
//   3. more than output_num components: the first output_num by (size descending, key ascending) stay (stable sort by size);
//   4. ratio = (output_num - G) / (n - G) in double, G = kept components; a kept one gives its 1 + floor(size * ratio) best members;
//   5. the picked candidates are ranked and cut to output_num.
// Ties: "best" and "ranked" mean the candidate's rank = its position in the input list (|d| ascending, then generation index). The
// score is non-increasing along the list, so on tie-free lists this is the host routine's result, row for row; where fp32 scores
// tie, the reference leaves the choice inside the run to std::partial_sort and the host routine takes member order.
//
// Kernels (all integer bookkeeping, so the result does not depend on scheduling):
//   cluster_init_kernel    fp32 boxes and areas (denet_samples_finish_host's arithmetic), union-find and counters reset
//   cluster_pairs_kernel   256 x 256 tiles over j < i, the j boxes of a tile in LDS, one i per thread: an edge marks has_earlier[i]
//                          and unions i and j in a lock-free union-find (larger root hooked under the smaller with atomicCAS, re-find
//                          on failure; no thread ever waits for another's progress)
//   cluster_label_kernel   label[i] = root = smallest index of the component; sizes (atomicAdd), keys (atomicMax over creators)
//   cluster_select_kernel  one workgroup per image: radix select of the kept components, takes, position of every member inside
//                          its component, compaction in rank order (wave ballots + prefix over the wave counts), cut, outputs
// Compiled with -ffp-contract=off.
#include "common.h"
#include "../../include/denet_hip.h"
#include <math.h>

namespace {

constexpr int TILE = 256;
constexpr int MAX_N = 61440;        // denet_build_samples' largest sample_count; sizes and keys then fit 16 bits each

struct Ws {
    size_t fbox, area, parent, flags, label, size, key, take, seen, total;
};

Ws ws_layout(int B, int N) {
    Ws l;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += (bytes + 255) & ~(size_t)255; return r; };
    const size_t rows = (size_t)B * N;
    l.fbox = take(rows * sizeof(float4));
    l.area = take(rows * sizeof(float));
    l.parent = take(rows * sizeof(int));
    l.flags = take(rows * sizeof(int));
    l.label = take(rows * sizeof(int));
    l.size = take(rows * sizeof(int));
    l.key = take(rows * sizeof(int));
    l.take = take(rows * sizeof(int));
    l.seen = take(rows * sizeof(int));
    l.total = o;
    return l;
}

struct Ctx {
    const int* box_in;      // [B][N][4]
    const float* absd_in;   // [B][N]
    const int* count_in;    // [B]
    float4* fbox;           // [B][N] x0, y0, x1, y1 as fp32 fractions
    float* area;            // [B][N]
    int* parent;            // [B][N] union-find
    int* flags;             // [B][N] has_earlier
    int* label;             // [B][N] smallest index of the component
    int* size;              // [B][N] at the root: members
    int* key;               // [B][N] at the root: youngest creator
    int* take;              // [B][N] at the root: members it contributes (0: component cut)
    int* seen;              // [B][N] at the root: members passed by the compaction so far
    int N, output_num, H, W;
    float thr;
};

// candidates of image b that take part: count clipped to the rows there are
__device__ __forceinline__ int image_count(const Ctx& c, int b) {
    const int n = c.count_in[b];
    return n < 0 ? 0 : (n > c.N ? c.N : n);
}

// values other threads of the grid change while this kernel runs are read and written through the L2
__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// root of x; parent[v] <= v everywhere, so the walk descends and ends. Path halving with atomicMin keeps the links monotone
__device__ __forceinline__ int uf_find(int* parent, int x) {
    int p = ld(parent + x);
    while (p != x) {
        const int g = ld(parent + p);
        if (g != p) atomicMin(parent + x, g);
        x = p;
        p = g;
    }
    return x;
}

// unions the sets of a and b, returns the root. A failed CAS means another thread hooked that root meanwhile (a root is hooked
// once, so the retries of all threads together are bounded by n): nobody waits for anybody
__device__ __forceinline__ int uf_unite(int* parent, int a, int b) {
    for (;;) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        if (atomicCAS(parent + a, a, b) == a) return b;
    }
}

__global__ __launch_bounds__(256) void cluster_init_kernel(Ctx c) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= c.N) return;
    const long r = (long)b * c.N + i;
    c.parent[r] = i;
    c.flags[r] = 0;
    c.size[r] = 0;
    c.key[r] = -1;
    c.take[r] = 0;
    c.seen[r] = 0;
    if (i < image_count(c, b)) {
        const int* bx = c.box_in + r * 4;
        // denet_samples_finish_host's box, as edit_samples_kernel forms it
        const float x0 = (float)((double)bx[0] / c.W);
        const float y0 = (float)((double)bx[1] / c.H);
        const float x1 = (float)((double)(bx[2] + 1) / c.W);
        const float y1 = (float)((double)(bx[3] + 1) / c.H);
        c.fbox[r] = make_float4(x0, y0, x1, y1);
        c.area[r] = (x1 - x0) * (y1 - y0);          // SampleType::area in fp32
    }
}

// is fp32 ai / au > thr, ai > 0. The quotient decides; a cheaper test stands in only where it provably agrees. With p = fl(thr * au)
// (relative error <= 2^-24) and one more rounding in p * (1 +- 2^-20):
//   ai > fl(p * (1 + 2^-20))  =>  ai / au > thr * (1 + 2^-20) * (1 - 2^-24)^2 > thr * (1 + 2^-21) > the float after thr  => quotient > thr
//   ai < fl(p * (1 - 2^-20))  =>  ai / au < thr * (1 - 2^-20) * (1 + 2^-24)^2 < thr * (1 - 2^-21) < the float before thr => quotient < thr
// (rounding is monotone; neighbouring floats are at most 2^-23 apart relatively). p must be a normal number for the error bounds:
// threshold 0, tiny thresholds and anything unexpected go through the quotient
__device__ __forceinline__ bool iou_above(float ai, float au, float thr) {
    const float p = thr * au;
    if (p > 1e-18f) {
        if (ai > p * 1.00000095367431640625f) return true;
        if (ai < p * 0.99999904632568359375f) return false;
    }
    return ai / au > thr;
}

__global__ __launch_bounds__(256) void cluster_pairs_kernel(Ctx c) {
    const int tj = blockIdx.x, ti = blockIdx.y, b = blockIdx.z;
    if (tj > ti) return;
    const int n = image_count(c, b);
    if (n <= c.output_num || ti * TILE >= n) return;
    __shared__ float4 lbox[TILE];
    __shared__ float larea[TILE];
    __shared__ int lhint[TILE];          // some node of j's component (a hint: equal hints = same component, for good)
    const long base = (long)b * c.N;
    int* parent = c.parent + base;
    const int tid = threadIdx.x;
    const int j0 = tj * TILE;
    const int jn = min(TILE, n - j0);
    if (tid < jn) {
        lbox[tid] = c.fbox[base + j0 + tid];
        larea[tid] = c.area[base + j0 + tid];
        lhint[tid] = ld(parent + j0 + tid);
    }
    __syncthreads();                     // the only barrier: threads may leave from here on
    const int i = ti * TILE + tid;
    if (i >= n) return;
    const float4 a = c.fbox[base + i];
    const float aa = c.area[base + i];
    int hint = ld(parent + i);
    bool earlier = false;
    const int jend = (ti == tj) ? min(jn, tid) : jn;        // j < i
    for (int jj = 0; jj < jend; ++jj) {
        const float4 q = lbox[jj];
        // SampleType::overlap / overlap_iou in fp32 (denet_sparse.cc:86-101)
        const float dx = fmaxf(0.0f, fminf(a.z, q.z) - fmaxf(a.x, q.x));
        const float dy = fmaxf(0.0f, fminf(a.w, q.w) - fmaxf(a.y, q.y));
        const float ai = dx * dy;
        if (!(ai > 0.0f)) continue;      // IoU 0 (or 0 / 0): never above a threshold >= 0
        const float au = aa + larea[jj] - ai;
        if (!iou_above(ai, au, c.thr)) continue;
        earlier = true;
        // dense clusters have O(n^2) edges: the union-find is touched only while the two are not known to be together
        if (((volatile int*)lhint)[jj] == hint) continue;
        hint = uf_unite(parent, i, j0 + jj);
        ((volatile int*)lhint)[jj] = hint;
    }
    if (earlier) c.flags[base + i] = 1;
}

__global__ __launch_bounds__(256) void cluster_label_kernel(Ctx c) {
    const int b = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n = image_count(c, b);
    if (n <= c.output_num || i >= n) return;
    const long base = (long)b * c.N;
    const int r = uf_find(c.parent + base, i);       // roots no longer change: the smallest index of the component
    c.label[base + i] = r;
    atomicAdd(c.size + base + r, 1);
    if (!c.flags[base + i]) atomicMax(c.key + base + r, i);
}

__global__ __launch_bounds__(1024) void cluster_select_kernel(Ctx c, int* __restrict__ box_out, float* __restrict__ absd_out,
                                                               int* __restrict__ count_out) {
    __shared__ unsigned hist[256];
    __shared__ int slab[1024];
    __shared__ int sh_w[16];
    __shared__ unsigned s_prefix, s_need;
    __shared__ int s_groups;
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = image_count(c, b);
    const int O = c.output_num;
    const long base = (long)b * c.N;
    const int* bin = c.box_in + base * 4;
    const float* din = c.absd_in + base;
    int* bo = box_out + (long)b * O * 4;
    float* dout = absd_out + (long)b * O;
    auto copy_row = [&](int dst, int src) {
        bo[dst * 4 + 0] = bin[src * 4 + 0]; bo[dst * 4 + 1] = bin[src * 4 + 1];
        bo[dst * 4 + 2] = bin[src * 4 + 2]; bo[dst * 4 + 3] = bin[src * 4 + 3];
        dout[dst] = din[src];
    };
    auto zero_rows = [&](int from) {
        for (int i = from + tid; i < O; i += 1024) {
            bo[i * 4 + 0] = bo[i * 4 + 1] = bo[i * 4 + 2] = bo[i * 4 + 3] = 0;
            dout[i] = 0.f;
        }
    };
    if (n <= O) {                        // the reference clusters only when there are more candidates than outputs
        for (int i = tid; i < n; i += 1024) copy_row(i, i);
        zero_rows(n);
        if (tid == 0) count_out[b] = n;
        return;
    }
    const int* label = c.label + base;
    const int* size = c.size + base;
    const int* key = c.key + base;
    int* take = c.take + base;
    int* seen = c.seen + base;

    // components
    if (tid == 0) s_groups = 0;
    __syncthreads();
    int mine = 0;
    for (int i = tid; i < n; i += 1024) mine += (label[i] == i);
    if (mine) atomicAdd(&s_groups, mine);
    __syncthreads();
    const int groups = s_groups;
    // order of the components: (size descending, key ascending) = ascending (n - size) << 16 | key, all distinct
    auto comp = [&](int i) { return ((unsigned)(n - size[i]) << 16) | (unsigned)key[i]; };
    unsigned T = 0xFFFFFFFFu;            // components with comp <= T stay
    if (groups > O) {
        if (tid == 0) { s_prefix = 0u; s_need = (unsigned)O; }
        for (int shift = 24; shift >= 0; shift -= 8) {
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix;
            const unsigned himask = (shift == 24) ? 0u : (0xFFFFFFFFu << (shift + 8));
            for (int i = tid; i < n; i += 1024) {
                if (label[i] != i) continue;
                const unsigned v = comp(i);
                if ((v & himask) == (prefix & himask)) atomicAdd(&hist[(v >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (tid == 0) {
                unsigned cum = 0, need = s_need;
                int sel = 255;
                for (int k = 0; k < 256; ++k) {
                    if (cum + hist[k] >= need) { sel = k; break; }
                    cum += hist[k];
                }
                s_need = need - cum;
                s_prefix = prefix | ((unsigned)sel << shift);
            }
            __syncthreads();
        }
        T = s_prefix;
    }
    const int kept = groups > O ? O : groups;
    // denet_sparse.cc:226-231
    const double ratio = (double)(O - kept) / (double)(n - kept);
    for (int i = tid; i < n; i += 1024) {
        if (label[i] != i) continue;
        take[i] = (comp(i) <= T) ? 1 + (int)floor((double)size[i] * ratio) : 0;
    }
    __syncthreads();

    // members in rank order, 1024 at a time: a member is picked while fewer than take[component] members of its component came
    // before it; the picked ones are compacted in order and cut to output_num
    int written = 0;
    for (int c0 = 0; c0 < n && written < O; c0 += 1024) {
        const int i = c0 + tid;
        const bool valid = i < n;
        const int L = valid ? label[i] : -1;
        slab[tid] = L;
        __syncthreads();
        const int tk = valid ? ld(take + L) : 0;
        bool pick = false;
        if (tk > 0) {
            const int before = ld(seen + L);
            if (before < tk) {
                int r = before;
                for (int t = 0; t < tid; ++t) r += (slab[t] == L);
                pick = r < tk;
            }
        }
        __syncthreads();                 // every thread has read `seen` before this chunk is added to it
        if (tk > 0) atomicAdd(seen + L, 1);
        const unsigned long long mask = __ballot(pick);
        const int wofs = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) sh_w[wave] = __popcll(mask);
        __syncthreads();
        int wbase = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            const int k = sh_w[w];
            if (w < wave) wbase += k;
            total += k;
        }
        if (pick) {
            const int dst = written + wbase + wofs;
            if (dst < O) copy_row(dst, i);
        }
        written += total;
        __syncthreads();
    }
    const int nout = written < O ? written : O;
    zero_rows(nout);
    if (tid == 0) count_out[b] = nout;
}

}  // namespace

extern "C" size_t denet_cluster_samples_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0 || N > MAX_N) return 0;
    return ws_layout(B, N).total;
}

extern "C" int denet_cluster_samples_device(const int* box_in, const float* absd_in, const int* count_in, int B, int N, float threshold,
                                            int output_num, int H, int W, int* box_out, float* absd_out, int* count_out,
                                            void* workspace, size_t workspace_bytes, hipStream_t stream) {
    DENET_CHECK_ARG(box_in && absd_in && count_in && box_out && absd_out && count_out && workspace, "cluster_samples_device: null pointer");
    DENET_CHECK_ARG(threshold >= 0.0f && threshold < 1.0f,
                    "cluster_samples_device: threshold %g is outside [0, 1): the closed form does not hold, use the host routine",
                    (double)threshold);
    DENET_CHECK_ARG(output_num > 0, "cluster_samples_device: output_num must be positive, got %d", output_num);
    DENET_CHECK_ARG(B > 0 && B <= 65535 && N > 0 && N <= MAX_N, "cluster_samples_device: B = %d, N = %d unsupported (N <= %d)", B, N, MAX_N);
    DENET_CHECK_ARG(H > 0 && W > 0 && H <= 256 && W <= 256, "cluster_samples_device: map %dx%d unsupported", H, W);
    const Ws l = ws_layout(B, N);
    DENET_CHECK_ARG(workspace_bytes >= l.total, "cluster_samples_device: N = %d rows need a workspace of %zu bytes, got %zu", N, l.total,
                    workspace_bytes);
    char* ws = (char*)workspace;
    Ctx c;
    c.box_in = box_in; c.absd_in = absd_in; c.count_in = count_in;
    c.fbox = (float4*)(ws + l.fbox); c.area = (float*)(ws + l.area); c.parent = (int*)(ws + l.parent);
    c.flags = (int*)(ws + l.flags); c.label = (int*)(ws + l.label); c.size = (int*)(ws + l.size); c.key = (int*)(ws + l.key);
    c.take = (int*)(ws + l.take); c.seen = (int*)(ws + l.seen);
    c.N = N; c.output_num = output_num; c.H = H; c.W = W; c.thr = threshold;
    const int tiles = (N + TILE - 1) / TILE;
    // ops.kernel_symbol: kinds 30..33 = the four launches, in this order
    int prof = denet_prof_begin(30, 0, 0, 0, stream);
    hipLaunchKernelGGL(cluster_init_kernel, dim3(tiles, B), dim3(256), 0, stream, c);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(31, 0, 0, 0, stream);
    hipLaunchKernelGGL(cluster_pairs_kernel, dim3(tiles, tiles, B), dim3(256), 0, stream, c);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(32, 0, 0, 0, stream);
    hipLaunchKernelGGL(cluster_label_kernel, dim3(tiles, B), dim3(256), 0, stream, c);
    denet_prof_end(prof, stream);
    prof = denet_prof_begin(33, 0, 0, 0, stream);
    hipLaunchKernelGGL(cluster_select_kernel, dim3(B), dim3(1024), 0, stream, c, box_out, absd_out, count_out);
    denet_prof_end(prof, stream);
    DENET_CHECK_LAUNCH("cluster_samples_device");
    return DENET_OK;
}
