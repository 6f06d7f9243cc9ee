// viewgeom.hip -- the view tools of python/depthmotionnet/dataset_tools/view_tools_cython.pyx for many ordered pairs of views at once:
// `_compute_visible_points_mask` (:9-58), `_compute_depth_ratios` (:108-159), and the counts that check_depth_consistency
// (view_tools.py:82-94) decides on.  The reference walks one depth map per call, one pixel at a time, on the host.
//
// A pixel (x, y) of view 1 is valid when its depth d is finite and > 0 (:35, :130).  Every operation below is ONE float32 rounding, in
// this order (:36-54, :131-149; gcc on baseline x86-64 has no FMA and evaluates a * b / c and a + b + c left to right):
//   X = (d * ((x + 0.5f) - cx)) / fx - t0      Y = (d * ((y + 0.5f) - cy)) / fy - t1      Z = d - t2
//   q_i = (RT[i][0] * X + RT[i][1] * Y) + RT[i][2] * Z                       RT = R1 transposed
//   p_i = ((P2[i][0] * q_0 + P2[i][1] * q_1) + P2[i][2] * q_2) + P2[i][3] * 1.0f
//   if p_2 > 0:  u = p_0 / p_2,  v = p_1 / p_2
// mask  (:55)       = u > bx && v > by && u < (float)(width2 - bx) && v < (float)(height2 - by)
// ratio (:150-157)  : if u > 0 && v > 0 && u < (float)W2 && v < (float)H2:
//                       x2 = clamp(round_half_even(u), 0, W2), y2 likewise with H2 -- W2 and H2 themselves, not W2 - 1: the reference
//                       reads depth2[y2, x2] with bounds checks off, i.e. flat element y2 * W2 + x2, which for x2 == W2 is the first
//                       pixel of the next row.  An element at or past H2 * W2 is outside the map: here that is "no ratio".
//                       d2 finite and > 0  ->  ratio = p_2 / d2
//                     every other pixel holds the quiet NaN 0x7fc00000 (np.full(..., np.nan), :124)
// The whole file is compiled with fp contraction OFF (the pragma below); `/` is hipcc's correctly rounded float32 division and rintf
// rounds half to even like Python's round(), which `int(round(v))` compiles to.  float32 denormals are kept (hipcc's default mode; the golden
// case with denormal intermediates comes out of the MI355X bit for bit like the reference).
//
// view_pairs_kernel<MASK, RATIO>: grid = (chunks of kViewChunk = 1024 pixels, pairs), one 256-lane workgroup per chunk, 4 consecutive
// pixels per lane (one 16-byte load where the plane is 16-byte aligned and the 4 pixels exist; scalar loads otherwise).  The pair's
// parameters are one record of kViewRecord floats (viewgeom.h), uniform over the workgroup.  MASK / RATIO say which per-pixel outputs
// are STORED -- every pixel of a stored output is written (0 / the NaN where the reference leaves its initial value); what is computed
// does not depend on them.  Each workgroup writes four int32 counts of its chunk (wave64 ballot + popcount per pixel slot, the 4 waves
// through LDS; no atomics):  valid1 | visible (mask == 1) | ratios (finite ratio) | consistent (finite ratio, lo < ratio < hi).
// view_counts_kernel: one workgroup per pair sums the chunk counts into counts[pair][4].
// All stores are plain C++ stores.
#include "viewgeom.h"

#pragma clang fp contract(off)

namespace demon {

typedef float vfloat4 __attribute__((ext_vector_type(4)));

namespace {

constexpr int kViewThreads = 256;
static_assert(kViewChunk == 4 * kViewThreads, "a lane holds 4 consecutive pixels");

__device__ __forceinline__ bool view_valid(float d) { return d > 0.0f && d < __builtin_inff(); }

}  // namespace

template <bool MASK, bool RATIO>
__global__ __launch_bounds__(kViewThreads) void view_pairs_kernel(ViewArgs a)
{
    __shared__ int wave_sum[kViewThreads / 64][4];
    const int pair = blockIdx.y, tid = threadIdx.x;
    const int p = (int)blockIdx.x * kViewChunk + 4 * tid;
    const float *P = a.records + (long)kViewRecord * pair;
    const float *plane1 = a.depth1 + (long)__float_as_int(P[36]) * a.plane1_stride;
    const float *plane2 = a.depth2 ? a.depth2 + (long)__float_as_int(P[37]) * a.plane2_stride : nullptr;

    // ---- the lane's 4 depths; pixels past the image read as 0 (invalid)
    vfloat4 d = {0.0f, 0.0f, 0.0f, 0.0f};
    if (p + 3 < a.hw && ((size_t)(plane1 + p) & 15) == 0) d = *(const vfloat4 *)(plane1 + p);
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p + j < a.hw) d[j] = plane1[p + j];
    }

    const float fx = P[0], cx = P[1], fy = P[2], cy = P[3];
    const float bx0 = P[28], by0 = P[29], bx1 = P[30], by1 = P[31], W2f = P[32], H2f = P[33], lo = P[34], hi = P[35];
    const int map2 = a.H2 * a.W2;
    const int y0 = p / a.w, x0 = p - y0 * a.w;

    unsigned vis[4];
    float ratio[4];
    int n_valid = 0, n_vis = 0, n_ratio = 0, n_cons = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        int x = x0 + j, y = y0;
        while (x >= a.w) { x -= a.w; ++y; }
        const bool ok = view_valid(d[j]);   // (0 past the image)
        const float px = (float)x + 0.5f, py = (float)y + 0.5f;
        const float X = (d[j] * (px - cx)) / fx - P[13];
        const float Y = (d[j] * (py - cy)) / fy - P[14];
        const float Z = d[j] - P[15];
        const float q0 = (P[4] * X + P[5] * Y) + P[6] * Z;
        const float q1 = (P[7] * X + P[8] * Y) + P[9] * Z;
        const float q2 = (P[10] * X + P[11] * Y) + P[12] * Z;
        const float pu = ((P[16] * q0 + P[17] * q1) + P[18] * q2) + P[19] * 1.0f;
        const float pv = ((P[20] * q0 + P[21] * q1) + P[22] * q2) + P[23] * 1.0f;
        const float pz = ((P[24] * q0 + P[25] * q1) + P[26] * q2) + P[27] * 1.0f;
        const bool front = ok && pz > 0.0f;
        const float u = pu / pz, v = pv / pz;
        const bool seen = front && u > bx0 && v > by0 && u < bx1 && v < by1;
        float r = __int_as_float(0x7fc00000);
        if (plane2 && front && u > 0.0f && v > 0.0f && u < W2f && v < H2f) {
            const int x2 = max(0, min(a.W2, (int)rintf(u))), y2 = max(0, min(a.H2, (int)rintf(v)));
            const int idx = y2 * a.W2 + x2;
            if (idx < map2) {
                const float d2 = plane2[idx];
                if (view_valid(d2)) r = pz / d2;
            }
        }
        const bool fin = fabsf(r) < __builtin_inff();   // false for the NaN
        vis[j] = seen ? 1u : 0u;
        ratio[j] = r;
        n_valid += __popcll(__ballot(ok));
        n_vis += __popcll(__ballot(seen));
        n_ratio += __popcll(__ballot(fin));
        n_cons += __popcll(__ballot(fin && r > lo && r < hi));
    }
    if ((tid & 63) == 0) {
        int *s = wave_sum[tid >> 6];
        s[0] = n_valid; s[1] = n_vis; s[2] = n_ratio; s[3] = n_cons;
    }
    __syncthreads();
    if (tid < 4)
        a.chunk_counts[((long)pair * a.chunks + blockIdx.x) * 4 + tid] = wave_sum[0][tid] + wave_sum[1][tid] + wave_sum[2][tid] + wave_sum[3][tid];

    if (p >= a.hw) return;
    if (MASK) {
        uint8_t *dst = a.mask + (long)pair * a.hw + p;
        if (p + 3 < a.hw && ((size_t)dst & 3) == 0) *(unsigned *)dst = vis[0] | vis[1] << 8 | vis[2] << 16 | vis[3] << 24;
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p + j < a.hw) dst[j] = (uint8_t)vis[j];
        }
    }
    if (RATIO) {
        float *dst = a.ratios + (long)pair * a.hw + p;
        if (p + 3 < a.hw && ((size_t)dst & 15) == 0) *(vfloat4 *)dst = vfloat4{ratio[0], ratio[1], ratio[2], ratio[3]};
        else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (p + j < a.hw) dst[j] = ratio[j];
        }
    }
}

__global__ __launch_bounds__(kViewThreads) void view_counts_kernel(ViewArgs a)
{
    __shared__ int wave_sum[kViewThreads / 64][4];
    const int pair = blockIdx.x, tid = threadIdx.x;
    int s[4] = {0, 0, 0, 0};
    for (int k = tid; k < a.chunks; k += kViewThreads) {
        const int *c = a.chunk_counts + ((long)pair * a.chunks + k) * 4;
#pragma unroll
        for (int i = 0; i < 4; ++i) s[i] += c[i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) s[i] += __shfl_xor(s[i], m);
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wave_sum[tid >> 6][i] = s[i];
    }
    __syncthreads();
    if (tid < 4) a.counts[4l * pair + tid] = wave_sum[0][tid] + wave_sum[1][tid] + wave_sum[2][tid] + wave_sum[3][tid];
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
bool view_shape_ok(int h, int w, int H2, int W2)
{
    // pixel indices, chunk counts and the flat lookup index (at most H2 * W2 + W2) are ints
    return h >= 1 && w >= 1 && (long)h * w <= (1l << 30) && H2 >= 1 && W2 >= 1 && (long)H2 * W2 <= (1l << 30);
}

int view_chunks(int h, int w) { return (int)(((long)h * w + kViewChunk - 1) / kViewChunk); }

void view_pack_record(const float *K1, const float *R1, const float *t1, const float *P2, int width2, int height2, int borderx, int bordery,
                      float lo, float hi, int plane1, int plane2, float *out)
{
    out[0] = K1[0]; out[1] = K1[2]; out[2] = K1[4]; out[3] = K1[5];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) out[4 + 3 * i + j] = R1[3 * j + i];
    for (int i = 0; i < 3; ++i) out[13 + i] = t1[i];
    for (int i = 0; i < 12; ++i) out[16 + i] = P2[i];
    // the int subtraction first, then the conversion, as C evaluates `u < width2 - borderx` (:55)
    out[28] = (float)borderx; out[29] = (float)bordery; out[30] = (float)(width2 - borderx); out[31] = (float)(height2 - bordery);
    out[32] = (float)width2; out[33] = (float)height2;
    out[34] = lo; out[35] = hi;
    static_assert(sizeof(int) == sizeof(float), "plane indices travel as bit patterns");
    __builtin_memcpy(out + 36, &plane1, sizeof(int));
    __builtin_memcpy(out + 37, &plane2, sizeof(int));
    out[38] = out[39] = 0.0f;
}

void launch_view_pairs(ViewArgs a, hipStream_t stream)
{
    a.hw = a.h * a.w;
    a.chunks = view_chunks(a.h, a.w);
    const dim3 grid((unsigned)a.chunks, (unsigned)a.n), block(kViewThreads);
    if (a.mask && a.ratios) hipLaunchKernelGGL((view_pairs_kernel<true, true>), grid, block, 0, stream, a);
    else if (a.mask) hipLaunchKernelGGL((view_pairs_kernel<true, false>), grid, block, 0, stream, a);
    else if (a.ratios) hipLaunchKernelGGL((view_pairs_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((view_pairs_kernel<false, false>), grid, block, 0, stream, a);
    hipLaunchKernelGGL(view_counts_kernel, dim3((unsigned)a.n), block, 0, stream, a);
}

}  // namespace demon
