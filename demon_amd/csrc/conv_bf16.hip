// conv_bf16.hip -- the implicit-GEMM convolution of conv_mfma.hip on the gfx950 bf16 matrix cores (option precision = 1).
//
// Same GEMM view, K table, tile shapes, split-K workspace and epilogue as conv_mfma.hip:
//   D[co][pix] = bias[co] + sum_k bf16(Wp[k][co]) * bf16(X[k][pix]),  accumulated in fp32
// Only the operands are rounded (round to nearest even); the products of two bf16 values are exact in fp32, bias, leaky relu, the
// depth scale and every store stay fp32.  Activations in HBM stay fp32: the B operand is gathered as fp32 and converted with a
// plain cast (v_cvt_pk_bf16_f32, which keeps NaN a NaN) on its way into LDS.
//
// v_mfma_f32_32x32x16_bf16: lane l feeds A[i = l&31][k = 8(l>>5) + j] and B[k = 8(l>>5) + j][col = l&31], j = 0..7, i.e. one
// 16-byte LDS read per operand per lane; its C/D layout is the one of v_mfma_f32_32x32x2_f32 (cdna_hip_programming.md section 3),
// so the epilogue is conv_mfma.hip's.
//   A: bf16 weights in global memory as [cls][Kb / 8][Mpad][8] (launch_bf16_repack, from the packed fp32 weights): one lane's 8 k
//      values of one output channel are one 16-byte chunk; the LDS image [k group][BM][8] is the same layout, copied as is.
//   B: [pixel][k] in LDS with a row pitch of BK + 8 bf16 (80 bytes): 16 consecutive rows fall on 16 different 16-byte bank slots,
//      so the ds_read_b128 fragment reads (lane groups of 16 rows) and the ds_write staging stores are free of bank conflicts.
// K-steps of BK = 32 (two MFMAs deep), one barrier per step on a double-buffered LDS tile; the gathers and weight loads of step s+1
// are in flight during the MFMAs of step s, the K table runs one step further ahead.  No atomics: results are deterministic.
#include <type_traits>

#include "internal.h"

namespace demon {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(64 * WM * WN) void conv_bf16_kernel(ConvArgs a, const bf16x8 *__restrict__ wb, long cls_wb_stride)
{
    constexpr int BK = kBf16K;
    constexpr int NT = 64 * WM * WN;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int KG = BK / 8;                 // 8-deep k groups per K-step
    constexpr int BROWS = NT / BN;             // k rows covered by one pass of the B staging
    constexpr int BPER = BK / BROWS;           // consecutive k of one pixel per thread per K-step
    constexpr int CH = BPER % 8 == 0 ? 8 : 4;  // bf16 per LDS store of the B staging
    constexpr int BPITCH = BK + 8;             // bf16 per pixel row of the B tile
    constexpr int ACH = KG * BM;               // 16-byte A chunks per K-step
    constexpr int APER = (ACH + NT - 1) / NT;
    static_assert(NT % BN == 0 && BK % BROWS == 0 && BPER % 4 == 0, "bad B staging shape");

    TlScope tl(a.tl);
    __shared__ __attribute__((aligned(16))) bf16x8 As[2][KG][BM];
    __shared__ __attribute__((aligned(16))) __bf16 Bs[2][BN][BPITCH];

    const int tid = threadIdx.x;
    const int cls = blockIdx.z / a.ksplit;
    const int zs = blockIdx.z - cls * a.ksplit;
    unsigned bx, by;
    xcd_tile(a.xcd, blockIdx.x, blockIdx.y, gridDim.x, gridDim.y, bx, by);
    const int m0 = by * BM;
    const long p0 = (long)bx * BN;
    const long P = (long)a.N * a.Hp * a.Wp;
    const bf16x8 *__restrict__ wcls = wb + (long)cls * cls_wb_stride;
    const KEntry *__restrict__ ktab = a.ktab + (long)cls * a.Kpad;

    // ---- B staging: this thread gathers k rows bg * BPER .. + BPER of pixel column bj
    const int bj = tid % BN;
    int bg = tid / BN;
    if (BN >= 64) bg = __builtin_amdgcn_readfirstlane(bg);  // wave-uniform: K table reads go scalar
    int iy0, ix0;
    const float *__restrict__ inb;
    {
        const long p = p0 + bj;
        if (p < P) {
            const int x = (int)(p % a.Wp);
            const long t = p / a.Wp;
            const int y = (int)(t % a.Hp);
            const int n = (int)(t / a.Hp);
            iy0 = y * a.sy;
            ix0 = x * a.sx;
            inb = a.in + (long)n * a.in_n_stride + (long)iy0 * a.W + ix0;
        } else {
            iy0 = -(1 << 20);  // every bounds test fails -> zeros
            ix0 = 0;
            inb = a.in;
        }
    }

    float breg[BPER];
    bf16x8 areg[APER];
    KEntry kentA[BPER], kentB[BPER];  // K-table entries, two K-steps in flight (even / odd step)
    unsigned okmask = 0;                 // bit i: B element i of the prefetched K-step is inside the image

    auto load_ktab = [&](KEntry (&k)[BPER], int step) {
        step = min(step, a.Kpad / BK - 1);  // the run-ahead may point past the table: re-read the last step
#pragma unroll
        for (int i = 0; i < BPER; ++i) k[i] = ktab[step * BK + bg * BPER + i];
    };
    // branch-free gather: out-of-image taps read the (always valid) anchor pixel and are zeroed when written to LDS
    auto gather = [&](const KEntry (&kent)[BPER]) {
        okmask = 0;
#pragma unroll
        for (int i = 0; i < BPER; ++i) {
            const int dy = kent[i].dydx >> 16;
            const int dx = (int)(short)(kent[i].dydx & 0xffff);
            const bool ok = ((unsigned)(iy0 + dy) < (unsigned)a.H) & ((unsigned)(ix0 + dx) < (unsigned)a.W);
            okmask |= (ok ? 1u : 0u) << i;
            breg[i] = inb[ok ? kent[i].delta : 0];
        }
    };
    auto load_a = [&](int step) {
#pragma unroll
        for (int i = 0; i < APER; ++i) {
            const int c = tid + i * NT;
            if (APER * NT == ACH || c < ACH) areg[i] = wcls[(long)(step * KG + c / BM) * a.Mpad + m0 + c % BM];
        }
    };
    auto store_tiles = [&](int buf) {
#pragma unroll
        for (int c = 0; c < BPER / CH; ++c) {
            typedef __bf16 chunk_t __attribute__((ext_vector_type(CH)));
            chunk_t v;
#pragma unroll
            for (int e = 0; e < CH; ++e) v[e] = (__bf16)(((okmask >> (c * CH + e)) & 1u) ? breg[c * CH + e] : 0.0f);
            *reinterpret_cast<chunk_t *>(&Bs[buf][bj][bg * BPER + c * CH]) = v;
        }
#pragma unroll
        for (int i = 0; i < APER; ++i) {
            const int c = tid + i * NT;
            if (APER * NT == ACH || c < ACH) As[buf][c / BM][c % BM] = areg[i];
        }
    };

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int l31 = lane & 31, lhi = lane >> 5;

    floatx16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;

    // the MFMAs of one K-step out of LDS buffer `buf`; with PREFETCH the table entries of step `ahead` are read behind the step's LDS
    // reads (a scalar-cache miss that an lgkmcnt wait of the fragment reads would otherwise sit out)
    auto compute = [&](int buf, int ahead, KEntry (&kent_load)[BPER], auto prefetch) {
        constexpr bool PREFETCH = decltype(prefetch)::value;
        bf16x8 av[KG / 2][TM], bv[KG / 2][TN];
#pragma unroll
        for (int kk = 0; kk < KG / 2; ++kk) {
            const int kg = 2 * kk + lhi;
#pragma unroll
            for (int i = 0; i < TM; ++i) av[kk][i] = As[buf][kg][(wm * TM + i) * 32 + l31];
#pragma unroll
            for (int j = 0; j < TN; ++j) bv[kk][j] = *reinterpret_cast<const bf16x8 *>(&Bs[buf][(wn * TN + j) * 32 + l31][kg * 8]);
        }
        if (PREFETCH) {
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0) only
            __builtin_amdgcn_sched_barrier(0);
            load_ktab(kent_load, ahead);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < KG / 2; ++kk)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(av[kk][i], bv[kk][j], acc[i][j], 0, 0, 0);
    };

    const int total_steps = a.Kpad / BK;
    const int per_slice = (total_steps + a.ksplit - 1) / a.ksplit;
    const int s_begin = zs * per_slice;
    const int nsteps = min(total_steps, s_begin + per_slice) - s_begin;  // may be <= 0 for a trailing slice
    // one K-step with a successor: the gathers and weight loads of step s+1 (table entries in kent_use) in flight during the MFMAs of
    // step s, the table entries of step s+2 read into kent_load
    auto step = [&](int s, const KEntry (&kent_use)[BPER], KEntry (&kent_load)[BPER]) {
        gather(kent_use);
        load_a(s_begin + s + 1);
        compute(s & 1, s_begin + s + 2, kent_load, std::true_type{});
        store_tiles((s + 1) & 1);
        __syncthreads();
    };
    if (nsteps > 0) {
        load_ktab(kentA, s_begin);
        gather(kentA);
        load_a(s_begin);
        load_ktab(kentB, s_begin + 1);
        store_tiles(0);
    }
    __syncthreads();
    tl.mark(1);
    // steps in pairs so that the table double buffer is indexed statically (as in conv_mfma.hip)
    int s = 0;
    for (; s + 2 < nsteps; s += 2) {
        step(s, kentB, kentA);
        step(s + 1, kentA, kentB);
    }
    if (s + 1 < nsteps) {
        step(s, kentB, kentA);
        ++s;
    }
    if (nsteps > 0) compute(s & 1, 0, kentA, std::false_type{});
    tl.mark(2);

    if (a.ksplit > 1) {  // raw partial sums to the workspace [cls][slice][Mpad][P]; conv_splitk_reduce finishes
        float *__restrict__ ws = a.ws + ((long)blockIdx.z * a.Mpad) * P;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const long p = p0 + (wn * TN + j) * 32 + l31;
            if (p >= P) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int co = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                    ws[(long)co * P + p] = acc[i][j][r];
                }
        }
        return;
    }
    // ---- epilogue (conv_mfma.hip's): bias, leaky relu, optional per-sample scale of channel 0, coalesced NCHW store
    const int pyc = cls >> 1, pxc = cls & 1;
    const long plane = a.out_plane;
    if (a.osx == 1 && a.osy == 1 && (a.Wp & 3) == 0 && (a.Cout & 3) == 0 && a.scale == nullptr) {
        const int q = l31 >> 2, li = lane & 3;
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const long p = p0 + (wn * TN + j) * 32 + 4 * q;
            const bool ok = p < P;
            const long pc = ok ? p : 0;
            const int x = (int)(pc % a.Wp);
            const long t = pc / a.Wp;
            const int y = (int)(t % a.Hp);
            const int n = (int)(t / a.Hp);
            float *__restrict__ ob = a.out + (long)n * a.out_n_stride + (long)y * a.Wo + x;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int rb = 0; rb < 4; ++rb) {
                    float v0 = acc[i][j][4 * rb + 0], v1 = acc[i][j][4 * rb + 1], v2 = acc[i][j][4 * rb + 2], v3 = acc[i][j][4 * rb + 3];
                    {
                        const bool odd = li & 1;  // exchange with the lane at distance 1 (quad_perm [1,0,3,2])
                        float s0 = odd ? v0 : v1, s1 = odd ? v2 : v3;
                        s0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s0), 0xB1, 0xF, 0xF, true));
                        s1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s1), 0xB1, 0xF, 0xF, true));
                        if (odd) { v0 = s0; v2 = s1; } else { v1 = s0; v3 = s1; }
                    }
                    {
                        const bool hi = li & 2;  // exchange with the lane at distance 2 (quad_perm [2,3,0,1])
                        float s0 = hi ? v0 : v2, s1 = hi ? v1 : v3;
                        s0 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s0), 0x4E, 0xF, 0xF, true));
                        s1 = __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, s1), 0x4E, 0xF, 0xF, true));
                        if (hi) { v0 = s0; v1 = s1; } else { v2 = s0; v3 = s1; }
                    }
                    const int co = m0 + (wm * TM + i) * 32 + li + 8 * rb + 4 * lhi;
                    if (ok && co < a.Cout) {
                        const float b = a.bias[co];
                        floatx4 v = {v0 + b, v1 + b, v2 + b, v3 + b};
                        if (a.act) {
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = v[e] >= 0.0f ? v[e] : 0.1f * v[e];
                        }
                        *reinterpret_cast<floatx4 *>(ob + (long)co * plane) = v;
                    }
                }
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const long p = p0 + (wn * TN + j) * 32 + l31;
        if (p >= P) continue;
        const int x = (int)(p % a.Wp);
        const long t = p / a.Wp;
        const int y = (int)(t % a.Hp);
        const int n = (int)(t / a.Hp);
        float *__restrict__ ob = a.out + (long)n * a.out_n_stride + (long)(y * a.osy + pyc) * a.Wo + (x * a.osx + pxc);
        const float sc = a.scale ? a.scale[n] : 1.0f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = m0 + (wm * TM + i) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
                if (co < a.Cout) {
                    float v = acc[i][j][r] + a.bias[co];
                    if (a.act) v = v >= 0.0f ? v : 0.1f * v;
                    if (co == 0) v *= sc;
                    ob[(long)co * plane] = v;
                }
            }
        }
    }
}

// packed fp32 weights [cls][Krows][Mpad] -> bf16 [cls][Kb / 8][Mpad][8] (rows k >= K are zero).  One thread per 16-byte chunk.
__global__ __launch_bounds__(256) void bf16_repack_kernel(bf16x8 *wb, const float *wp, int ncls, int K, int Kb, int Mpad, long cls_w_stride)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long per_cls = (long)(Kb / 8) * Mpad;
    if (idx >= ncls * per_cls) return;
    const int cls = (int)(idx / per_cls);
    const long r = idx - cls * per_cls;
    const int kg = (int)(r / Mpad), m = (int)(r % Mpad);
    const float *src = wp + cls * cls_w_stride + m;
    bf16x8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int k = kg * 8 + j;
        v[j] = (__bf16)(k < K ? src[(long)k * Mpad] : 0.0f);
    }
    wb[idx] = v;
}

void launch_bf16_repack(void *wb, const float *wp, int ncls, int K, int Kb, int Mpad, long cls_w_stride, hipStream_t s)
{
    const long chunks = (long)ncls * (Kb / 8) * Mpad;
    hipLaunchKernelGGL(bf16_repack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, (bf16x8 *)wb, wp, ncls, K, Kb, Mpad, cls_w_stride);
}

struct TileInfo { int bm, bn; float eff; };
static const TileInfo kTiles[TILE_COUNT] = {   // the shapes and order of conv_mfma.hip (enum ConvTile)
    {128, 128, 1.00f}, {64, 128, 0.95f}, {32, 128, 0.80f}, {64, 64, 0.85f},
    {32, 64, 0.65f},   {32, 32, 0.45f},  {128, 32, 0.80f}, {64, 32, 0.65f},
};

// choose_conv_plan's rule on the bf16 K-steps: the largest tile that fits, split-K until about two workgroups per CU exist
ConvPlan choose_bf16_plan(int Mpad, long pixels, int nclasses, int Kb, long ws_floats)
{
    const int nsteps = Kb / kBf16K;
    ConvPlan best{TILE_32x32, 1};
    float best_score = -1.0f;
    for (int t = 0; t < TILE_COUNT; ++t) {
        const TileInfo &ti = kTiles[t];
        if (Mpad % ti.bm) continue;
        if (ti.bn > 32 && pixels * 2 <= ti.bn) continue;
        const long wgs = (long)(Mpad / ti.bm) * ((pixels + ti.bn - 1) / ti.bn) * nclasses;
        int split = 1;
        if (wgs < 384) {
            split = (int)((512 + wgs - 1) / wgs);
            const int smax = nsteps / 4 > 1 ? nsteps / 4 : 1;
            if (split > smax) split = smax;
            while (split > 1 && (long)nclasses * split * Mpad * pixels > ws_floats) --split;
        }
        float fill = (float)(wgs * split) / 512.0f;
        if (fill > 1.0f) fill = 1.0f;
        const float score = ti.eff * fill / (1.0f + 0.12f * (split - 1));
        if (score > best_score) { best_score = score; best = ConvPlan{t, split}; }
    }
    return best;
}

template <int BM, int BN, int WM, int WN>
static void launch_tile(const ConvArgs &a, const void *wb, long cls_wb_stride, dim3 grid, hipStream_t stream)
{
    hipLaunchKernelGGL((conv_bf16_kernel<BM, BN, WM, WN>), grid, dim3(64 * WM * WN), 0, stream, a, (const bf16x8 *)wb, cls_wb_stride);
}

void launch_conv_bf16(const ConvArgs &a_in, const void *wb, ConvPlan plan, int nclasses, hipStream_t stream)
{
    ConvArgs a = a_in;
    a.ksplit = plan.ksplit;
    const long P = (long)a.N * a.Hp * a.Wp;
    const long cls_wb_stride = (long)(a.Kpad / 8) * a.Mpad;   // in 16-byte chunks
    const TileInfo ti = kTiles[plan.tile];
    dim3 grid((unsigned)((P + ti.bn - 1) / ti.bn), (unsigned)(a.Mpad / ti.bm), (unsigned)(nclasses * plan.ksplit));
    switch (plan.tile) {
        case TILE_128x128: launch_tile<128, 128, 2, 2>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_64x128:  launch_tile<64, 128, 2, 2>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_32x128:  launch_tile<32, 128, 1, 4>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_64x64:   launch_tile<64, 64, 2, 2>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_32x64:   launch_tile<32, 64, 1, 2>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_128x32:  launch_tile<128, 32, 4, 1>(a, wb, cls_wb_stride, grid, stream); break;
        case TILE_64x32:   launch_tile<64, 32, 2, 1>(a, wb, cls_wb_stride, grid, stream); break;
        default:           launch_tile<32, 32, 1, 1>(a, wb, cls_wb_stride, grid, stream); break;
    }
    if (plan.ksplit > 1) launch_splitk_reduce(a, nclasses, stream);
}

}  // namespace demon
