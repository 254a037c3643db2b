// The two sparsifiers that build the fourth input plane from the LIDAR map, on the already staged depth planes of a batch
// (the reference: dataset/dense_to_sparse.py, get_sparse_depth in dataset/nuscenes_dataset_torch_new.py:200-216).
//   lidar_radar   LidarRadarSampling: for every radar pixel (radar > 0) the two lidar pixels (lidar > 0) nearest to it; the plane is
//                 the lidar depth at the union of those pixels.
//     collect_kernel      one pass over the batch: every radar / lidar pixel is appended as (row << 16 | column) to its frame's list
//                         in the workspace (one integer atomicAdd per wavefront, list and run of 2048 pixels), and the output plane is
//                         cleared by the thread that has read the same pixels' radar values, so the plane may be the radar plane.
//     nearest_kernel      one wavefront per radar pixel, a persistent grid looping on the device-side counts: lanes stride over the
//                         frame's lidar list, each keeping its two smallest keys (d^2 << 32 | linear index); two rounds of a wave-wide
//                         minimum merge them and lane 0 copies the two winners' depth.  Keys are unique integers, so the result does
//                         not depend on the order the lists were filled in; several radar pixels picking one lidar pixel store the
//                         same value.
//   uniform       UniformSampling: keep = depth > 0 && depth <= (float)max_depth, prob = num_samples / count(keep) in float64, the plane
//                 is depth where keep && U < prob, U the caller's float64 draws or Philox4x32-10 (see the header).
//     count_kernel        per-frame count of keep: wave-wide integer sums, one integer atomicAdd per workgroup
//     sample_kernel       one streaming pass: IEEE float64 division, strict <, plane and optional mask
// Counts never reach the host.  No floating-point atomics; the only LDS and barrier are count_kernel's four partial sums;
// contraction is off for the whole file.
#include "common.h"

#include <algorithm>
#include <math.h>

#pragma clang fp contract(off)

namespace rd {

// the head of the workspace: one record per frame, then the radar lists [B][H*W] and the lidar lists [B][H*W]
struct SparseCounts { int32_t n_radar, n_lidar, n_keep, pad_; };

constexpr int kMaxSide = 46340;                     // 2 * (kMaxSide - 1)^2 < 2^32: a squared pixel distance fits the key's upper word
constexpr unsigned long long kNoKey = ~0ull;        // an empty slot: after every real key

static inline int64_t counts_bytes(int B) { return ((int64_t)B * (int64_t)sizeof(SparseCounts) + 255) / 256 * 256; }

// Pixels per wavefront and list append in collect_kernel: kRun chunks of 64.  Atomics on one frame's counter serialise, so a wave
// gathers the hits of a long run and reserves their places with one atomicAdd per list.
constexpr int kRun = 32;
constexpr int kBlock = 256;                         // threads of every launch here: four wavefronts (count_kernel's part[] relies on it)

// One chunk's hits: this lane's place among the wave's hits so far (or -1), and the running total (wave-uniform).
__device__ __forceinline__ int wave_place(bool hit, int& total) {
    const unsigned long long m = __ballot(hit);
    const int place = hit ? total + __popcll(m & ((1ull << (threadIdx.x & 63)) - 1)) : -1;
    total += __popcll(m);
    return place;
}

// The wave's `total` places in a list: one atomicAdd by lane 0, the base broadcast.  Every lane of the wave calls this together.
__device__ __forceinline__ int wave_reserve(int32_t* __restrict__ counter, int total) {
    int base = 0;
    if (total == 0) return 0;                                                    // wave-uniform
    if ((threadIdx.x & 63) == 0) base = atomicAdd(counter, total);
    return __shfl(base, 0, 64);
}

__global__ __launch_bounds__(kBlock) void collect_kernel(const float* __restrict__ lidar, int64_t lidar_stride, const float* radar,
                                                      int64_t radar_stride, int W, int n, SparseCounts* __restrict__ cnt,
                                                      uint32_t* __restrict__ rlist, uint32_t* __restrict__ llist, float* out, int64_t out_stride) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int64_t start = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 * kRun);      // this wave's run of frame b
    if (start >= n) return;                                                     // wave-uniform, and the kernel has no barrier
    const float* lb = lidar + (int64_t)b * lidar_stride;
    const float* rb = radar + (int64_t)b * radar_stride;
    float* ob = out + (int64_t)b * out_stride;
    float lv[kRun], rv[kRun];
#pragma unroll
    for (int k = 0; k < kRun; ++k) {                                            // every read of this thread before any of its writes:
        const int64_t e = start + k * 64 + lane;                                // out may be the radar plane, and the loads stay in flight
        lv[k] = e < n ? lb[e] : 0.f;
        rv[k] = e < n ? rb[e] : 0.f;
    }
    int place_r[kRun], place_l[kRun], total_r = 0, total_l = 0;
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        const int64_t e = start + k * 64 + lane;
        if (e < n) ob[e] = 0.f;
        place_r[k] = wave_place(rv[k] > 0.f, total_r);
        place_l[k] = wave_place(lv[k] > 0.f, total_l);
    }
    const int base_r = wave_reserve(&cnt[b].n_radar, total_r), base_l = wave_reserve(&cnt[b].n_lidar, total_l);
    uint32_t* rl = rlist + (int64_t)b * n;
    uint32_t* ll = llist + (int64_t)b * n;
#pragma unroll
    for (int k = 0; k < kRun; ++k) {
        if (place_r[k] < 0 && place_l[k] < 0) continue;
        const int e = (int)start + k * 64 + lane, y = e / W;
        const uint32_t yx = ((uint32_t)y << 16) | (uint32_t)(e - y * W);
        if (place_r[k] >= 0) rl[base_r + place_r[k]] = yx;
        if (place_l[k] >= 0) ll[base_l + place_l[k]] = yx;
    }
}

__global__ __launch_bounds__(kBlock) void nearest_kernel(const float* __restrict__ lidar, int64_t lidar_stride, int B, int W, int n,
                                                      const SparseCounts* __restrict__ cnt, const uint32_t* __restrict__ rlist,
                                                      const uint32_t* __restrict__ llist, float* __restrict__ out, int64_t out_stride) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    for (int b = 0; b < B; ++b) {
        const int nr = min(max(cnt[b].n_radar, 0), n), nl = min(max(cnt[b].n_lidar, 0), n);      // (never outside the lists)
        if (nl == 0) continue;
        const uint32_t* rl = rlist + (int64_t)b * n;
        const uint32_t* ll = llist + (int64_t)b * n;
        const int rot = (int)(((int64_t)b * n_waves) / B);                     // frame b starts at another wave: small frames spread out
        for (int r = wave - rot + (wave < rot ? n_waves : 0); r < nr; r += n_waves) {
            const uint32_t p = rl[r];
            const int py = (int)(p >> 16), px = (int)(p & 0xffffu);
            unsigned long long k0 = kNoKey, k1 = kNoKey;
            for (int j = lane; j < nl; j += 64) {
                const uint32_t q = ll[j];
                const int qy = (int)(q >> 16), qx = (int)(q & 0xffffu);
                const int dy = qy - py, dx = qx - px;
                const uint32_t d2 = (uint32_t)(dy * dy) + (uint32_t)(dx * dx);
                const unsigned long long key = ((unsigned long long)d2 << 32) | (uint32_t)(qy * W + qx);
                if (key < k1) {
                    if (key < k0) k1 = k0, k0 = key;
                    else k1 = key;
                }
            }
            unsigned long long win[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                unsigned long long m = k0;
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const unsigned long long other = __shfl_xor(m, o, 64);
                    m = other < m ? other : m;
                }
                win[k] = m;
                if (m != kNoKey && k0 == m) k0 = k1, k1 = kNoKey;                // keys are unique: one owner pops its head
            }
            if (lane == 0) {
                const float* lb = lidar + (int64_t)b * lidar_stride;
                float* ob = out + (int64_t)b * out_stride;
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const uint32_t idx = (uint32_t)(win[k] & 0xffffffffull);
                    if (win[k] != kNoKey && idx < (uint32_t)n) ob[idx] = lb[idx];
                }
            }
        }
    }
}

__device__ __forceinline__ bool keep_pixel(float v, float max_depth) { return v > 0.f && v <= max_depth; }

// One integer atomicAdd per workgroup: wave-wide sums, then the four waves' sums through LDS.
__global__ __launch_bounds__(kBlock) void count_kernel(const float* __restrict__ depth, int64_t depth_stride, int n, float max_depth,
                                                    SparseCounts* __restrict__ cnt) {
    __shared__ int part[kBlock / 64];
    static_assert(kBlock == 256, "the sum below reads four partial sums");
    const int b = blockIdx.y;
    const float* db = depth + (int64_t)b * depth_stride;
    int c = 0;
#pragma unroll 8
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) c += keep_pixel(db[e], max_depth);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    rd_sync();                                                                  // reached by every thread of the block
    if (threadIdx.x != 0) return;
    const int total = part[0] + part[1] + part[2] + part[3];
    if (total) atomicAdd(&cnt[b].n_keep, total);
}

__device__ __forceinline__ void philox_round(uint32_t& c0, uint32_t& c1, uint32_t& c2, uint32_t& c3, uint32_t k0, uint32_t k1) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0, c1 = lo1, c2 = hi0 ^ c3 ^ k1, c3 = lo0;
}

// Philox4x32-10 of counter (pixel, frame low, frame high, 0) under key (seed low, seed high); numpy's 53-bit double from x0, x1
__device__ __forceinline__ double philox_uniform(uint32_t pixel, unsigned long long frame, unsigned long long seed) {
    uint32_t c0 = pixel, c1 = (uint32_t)frame, c2 = (uint32_t)(frame >> 32), c3 = 0;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        philox_round(c0, c1, c2, c3, k0, k1);
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return ((double)(c0 >> 5) * 67108864.0 + (double)(c1 >> 6)) * (1.0 / 9007199254740992.0);
}

__global__ __launch_bounds__(kBlock) void sample_kernel(const float* depth, int64_t depth_stride, int n, double num_samples, float max_depth,
                                                     const double* __restrict__ draws, unsigned long long seed, unsigned long long frame0,
                                                     const SparseCounts* __restrict__ cnt, float* out, int64_t out_stride,
                                                     uint8_t* __restrict__ mask) {
    const int b = blockIdx.y;
    const float* db = depth + (int64_t)b * depth_stride;
    float* ob = out + (int64_t)b * out_stride;
    const int n_keep = cnt[b].n_keep;
    const double prob = n_keep > 0 ? num_samples / (double)n_keep : 0.0;        // n_keep == 0: nothing is kept and nothing is divided
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < n; e += gridDim.x * blockDim.x) {
        const float v = db[e];
        bool m = n_keep > 0 && keep_pixel(v, max_depth);
        if (m) m = (draws ? draws[(int64_t)b * n + e] : philox_uniform((uint32_t)e, frame0 + (unsigned long long)b, seed)) < prob;
        ob[e] = m ? v : 0.f;                                                    // after this thread's own read: out may be the depth plane
        if (mask) mask[(int64_t)b * n + e] = m;
    }
}

static int check_planes(const char* what, int B, int H, int W) {
    RD_CHECK_CODE(B >= 1 && B <= 65535 && H >= 1 && H <= kMaxSide && W >= 1 && W <= kMaxSide, RD_ESPARSE_RANGE,
                  "%s: B=%d (1..65535) frame %dx%d (sides 1..%d)", what, B, H, W, kMaxSide);
    RD_CHECK_CODE((int64_t)H * W < (1ll << 30), RD_ESPARSE_PIXELS, "%s: frame %dx%d has 2^30 pixels or more", what, H, W);
    return RD_OK;
}

// Whether a frame of plane a shares memory with a frame of plane b (B frames of n floats each, sa / sb floats apart).  Exact for equal
// strides (planes of one tensor: only the two frame offsets nearest to the distance can touch); for different strides the two
// extents are compared, which may call interleaved planes overlapping.
static bool planes_overlap(const float* a, int64_t sa, const float* b, int64_t sb, int B, int n) {
    const int64_t pa = (int64_t)reinterpret_cast<intptr_t>(a), pb = (int64_t)reinterpret_cast<intptr_t>(b);
    const int64_t N = (int64_t)n * 4, ea = ((int64_t)(B - 1) * sa + n) * 4, eb = ((int64_t)(B - 1) * sb + n) * 4;
    if (pa + ea <= pb || pb + eb <= pa) return false;
    if (sa != sb) return true;
    const int64_t S = sa * 4, d = pb - pa;
    int64_t k = d / S;
    if (d % S < 0) --k;                                                         // floor
    for (int64_t j = k; j <= k + 1; ++j)
        if (j > -B && j < B && d - j * S > -N && d - j * S < N) return true;
    return false;
}

// the grid of the grid-stride kernels, one row of blocks per frame: `per_cu` blocks a CU over the whole grid, `per_block` pixels a
// block at least
static dim3 stream_grid(int B, int n, int per_cu, int per_block) {
    return dim3((int)std::min<int64_t>(cdiv64(n, per_block), std::max(1, num_cus() * per_cu / B)), B);
}

}  // namespace rd
using namespace rd;

extern "C" int64_t rd_lidar_sparsify_workspace_bytes(int32_t B, int32_t H, int32_t W) {
    if (check_planes("lidar_sparsify_workspace_bytes", B, H, W)) return RD_EINVAL;
    return counts_bytes(B) + 2 * (int64_t)B * H * W * (int64_t)sizeof(uint32_t);
}

extern "C" int rd_lidar_radar_sparsify(const float* lidar, int64_t lidar_stride, const float* radar, int64_t radar_stride, int32_t B, int32_t H,
                                       int32_t W, void* workspace, float* out, int64_t out_stride, void* stream) {
    RD_CHECK_CODE(lidar && radar && workspace && out, RD_ESPARSE_NULL, "lidar_radar_sparsify: null argument");
    if (const int rc = check_planes("lidar_radar_sparsify", B, H, W)) return rc;
    const int n = H * W;
    RD_CHECK_CODE(lidar_stride >= n && radar_stride >= n && out_stride >= n, RD_ESPARSE_STRIDE,
                  "lidar_radar_sparsify: batch strides %lld / %lld / %lld below the %d pixels of a frame", (long long)lidar_stride,
                  (long long)radar_stride, (long long)out_stride, n);
    RD_CHECK_CODE(!planes_overlap(lidar, lidar_stride, out, out_stride, B, n), RD_ESPARSE_OVERLAP,
                  "lidar_radar_sparsify: out overlaps the lidar plane, which is read after out has been cleared");
    RD_CHECK_CODE((out == radar && out_stride == radar_stride) || !planes_overlap(radar, radar_stride, out, out_stride, B, n), RD_ESPARSE_OVERLAP,
                  "lidar_radar_sparsify: out overlaps the radar plane without being that plane");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SparseCounts* cnt = static_cast<SparseCounts*>(workspace);
    uint32_t* rlist = reinterpret_cast<uint32_t*>(static_cast<char*>(workspace) + counts_bytes(B));
    uint32_t* llist = rlist + (int64_t)B * n;
    RD_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)counts_bytes(B), s));
    hipLaunchKernelGGL(collect_kernel, dim3((int)cdiv64(n, kBlock * kRun), B), dim3(kBlock), 0, s, lidar, lidar_stride, radar, radar_stride, W, n, cnt, rlist, llist, out,
                       out_stride);
    RD_CHECK_LAUNCH("collect_kernel");
    hipLaunchKernelGGL(nearest_kernel, dim3(std::max(1, num_cus() * 8)), dim3(kBlock), 0, s, lidar, lidar_stride, B, W, n, cnt, rlist, llist, out,
                       out_stride);
    RD_CHECK_LAUNCH("nearest_kernel");
    return RD_OK;
}

extern "C" int rd_uniform_sparsify(const float* depth, int64_t depth_stride, int32_t B, int32_t H, int32_t W, int64_t num_samples, double max_depth,
                                   const double* draws, uint64_t seed, uint64_t frame0, void* workspace, float* out, int64_t out_stride,
                                   uint8_t* mask, void* stream) {
    RD_CHECK_CODE(depth && workspace && out, RD_ESPARSE_NULL, "uniform_sparsify: null argument");
    if (const int rc = check_planes("uniform_sparsify", B, H, W)) return rc;
    const int n = H * W;
    RD_CHECK_CODE(depth_stride >= n && out_stride >= n, RD_ESPARSE_STRIDE, "uniform_sparsify: batch strides %lld / %lld below the %d pixels of a frame",
                  (long long)depth_stride, (long long)out_stride, n);
    RD_CHECK_CODE(num_samples >= 0, RD_ESPARSE_SAMPLES, "uniform_sparsify: num_samples %lld is negative", (long long)num_samples);
    RD_CHECK_CODE(max_depth == max_depth, RD_ESPARSE_MAXDEPTH, "uniform_sparsify: max_depth is NaN");
    RD_CHECK_CODE((out == depth && out_stride == depth_stride) || !planes_overlap(depth, depth_stride, out, out_stride, B, n), RD_ESPARSE_OVERLAP,
                  "uniform_sparsify: out overlaps the depth plane without being that plane");
    hipStream_t s = static_cast<hipStream_t>(stream);
    SparseCounts* cnt = static_cast<SparseCounts*>(workspace);
    const float md = (float)max_depth;              // torch compares an fp32 tensor with a Python float in fp32
    RD_CHECK_HIP(hipMemsetAsync(cnt, 0, (size_t)counts_bytes(B), s));
    hipLaunchKernelGGL(count_kernel, stream_grid(B, n, 4, kBlock * 8), dim3(kBlock), 0, s, depth, depth_stride, n, md, cnt);
    RD_CHECK_LAUNCH("count_kernel");
    hipLaunchKernelGGL(sample_kernel, stream_grid(B, n, 16, 1024), dim3(kBlock), 0, s, depth, depth_stride, n, (double)num_samples, md, draws,
                       (unsigned long long)seed, (unsigned long long)frame0, cnt, out, out_stride, mask);
    RD_CHECK_LAUNCH("sample_kernel");
    return RD_OK;
}
