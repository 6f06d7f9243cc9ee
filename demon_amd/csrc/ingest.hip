// ingest.hip -- uint8 image pairs to the networks' inputs in one launch: what examples/example.py:15-42 (`prepare_input_data`) does on
// the host with PIL and numpy.  Two staged batches of RGB images [N][src_h][src_w][3] become
//   image_pair [N][6][H][W]      = [R1 G1 B1 R2 G2 B2], each image resized to H x W with Pillow's NEAREST rule
//   image2_2   [N][3][H/4][W/4]  = the RESIZED second image resized again by NEAREST (ratio exactly 4: row 4 y + 2, column 4 x + 2)
// with every value (float)v / 255.0f - 0.5f: an IEEE float32 division, then a float32 subtraction (no reciprocal multiply; the file
// is built without fast-math, and hipcc's fp32 division is correctly rounded by default).  A workgroup computes the 256 possible
// results once, by exactly these two operations, into LDS while its source loads are in flight, and every value is a table read: the
// correctly rounded division expands to about a dozen vector instructions, 24 times per lane (measured at batch 32, identity size:
// 13.4 us with the divisions in line, 13.0 us with the table).
//
// The source row / column of an output row / column comes from two index tables built on the host (ingest_index_table: Pillow
// accumulates a double-precision running sum, which no closed form reproduces for every size -- DESIGN.md).
//
// 4 bytes out per 1 or 3 bytes in: the kernel is bound by its stores.  A lane produces 4 consecutive pixels of a row and stores one
// 16-byte vector per plane (a wave: 1 KiB contiguous per plane).  grid.y = image of the batch; grid.x = the blocks of the full-size
// planes (H W / 4 lanes, a whole number of blocks since H and W are multiples of 32), then the blocks of the quarter-size planes.
//   identity (src == dst): the 12 source bytes of 4 pixels are 3 aligned dwords at byte 12 i of the image
//   resize: source rows start at 3 src_w-byte offsets, i.e. anywhere -- byte loads per channel, the 4 column indices as one 16-byte
//           load of the table (L1 / L2 resident: W ints)
// Every access goes through a buffer resource of the true extent: one staged image, one table, one sample of an output.
#include "internal.h"

namespace demon {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// the 256 values, computed while the workgroup's source loads are in flight (called by every lane of the workgroup)
__device__ __forceinline__ void ingest_fill_lut(float *lut)
{
    for (int v = threadIdx.x; v < 256; v += blockDim.x) lut[v] = (float)v / 255.0f - 0.5f;
    __syncthreads();
}

// byte `b` (0..3) of `w` through the table
__device__ __forceinline__ float ingest_byte(const float *lut, unsigned w, int b) { return lut[(w >> (8 * b)) & 255u]; }

template <bool IDENT>
__global__ __launch_bounds__(256) void ingest_kernel(IngestArgs a)
{
    __shared__ float lut[256];
    const int n = blockIdx.y;
    const int HW = a.H * a.W, img_bytes = 3 * a.src_h * a.src_w;
    const auto src1 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.img1 + (long)n * img_bytes), 0, img_bytes, 0x00020000);
    const auto src2 = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(a.img2 + (long)n * img_bytes), 0, img_bytes, 0x00020000);
    const auto rows = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(a.rowtab), 0, 4 * a.H, 0x00020000);
    const auto cols = __builtin_amdgcn_make_buffer_rsrc(const_cast<int *>(a.coltab), 0, 4 * a.W, 0x00020000);

    if ((int)blockIdx.x < a.full_blocks) {
        // ---- full size: lane i = pixels 4 i .. 4 i + 3 of the H x W plane, both images
        const int i = blockIdx.x * blockDim.x + threadIdx.x;
        unsigned px[2][4][3];   // [image][pixel][channel]: the byte itself, or the dword that holds it (identity)
        if (IDENT) {
#pragma unroll
            for (int k = 0; k < 2; ++k)
#pragma unroll
                for (int d = 0; d < 3; ++d) px[k][0][d] = __builtin_amdgcn_raw_buffer_load_b32(k ? src2 : src1, 12 * i + 4 * d, 0, 0);
        } else {
            const int W4 = a.W >> 2, y = i / W4, xq = i - y * W4;
            const int row = a.src_w * (int)__builtin_amdgcn_raw_buffer_load_b32(rows, 4 * y, 0, 0);
            const u32x4 cx = __builtin_amdgcn_raw_buffer_load_b128(cols, 16 * xq, 0, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int off = 3 * (row + (int)cx[j]);
#pragma unroll
                for (int k = 0; k < 2; ++k)
#pragma unroll
                    for (int c = 0; c < 3; ++c) px[k][j][c] = __builtin_amdgcn_raw_buffer_load_b8(k ? src2 : src1, off + c, 0, 0);
            }
        }
        ingest_fill_lut(lut);
        const auto out = __builtin_amdgcn_make_buffer_rsrc(a.pair + (long)n * a.pair_n_stride, 0, 4 * 6 * HW, 0x00020000);
#pragma unroll
        for (int k = 0; k < 2; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                floatx4 v;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int b = 3 * j + c;   // identity: byte b of the 12 loaded ones
                    v[j] = IDENT ? ingest_byte(lut, px[k][0][b >> 2], b & 3) : lut[px[k][j][c]];
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out, 4 * ((3 * k + c) * HW + 4 * i), 0, 0);
            }
    } else {
        // ---- quarter size: lane q = pixels 4 q .. 4 q + 3 of the H/4 x W/4 plane, second image only, through BOTH tables
        const int q = (blockIdx.x - a.full_blocks) * blockDim.x + threadIdx.x;
        const int HW2 = HW >> 4;
        const bool ok = 4 * q < HW2;   // the last workgroup's spare lanes: loads return 0 and stores are dropped by the range check
        constexpr int OOB = 0x7ffffff0;
        const int W16 = a.W >> 4, y = q / W16, xq = q - y * W16;
        const int row = a.src_w * (int)__builtin_amdgcn_raw_buffer_load_b32(rows, ok ? 4 * (4 * y + 2) : OOB, 0, 0);
        unsigned px[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int off = 3 * (row + (int)__builtin_amdgcn_raw_buffer_load_b32(cols, ok ? 4 * (16 * xq + 4 * j + 2) : OOB, 0, 0));
#pragma unroll
            for (int c = 0; c < 3; ++c) px[j][c] = __builtin_amdgcn_raw_buffer_load_b8(src2, ok ? off + c : OOB, 0, 0);
        }
        ingest_fill_lut(lut);
        const auto out = __builtin_amdgcn_make_buffer_rsrc(a.img22 + (long)n * a.img22_n_stride, 0, 4 * 3 * HW2, 0x00020000);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            floatx4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = lut[px[j][c]];
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), out, ok ? 4 * (c * HW2 + 4 * q) : OOB, 0, 0);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// Pillow's NEAREST resize along one axis: the source index of output sample x is the truncated running sum xo = a0 / 2 + x a0 in
// double precision, accumulated by additions.  floor((x + 0.5) src / dst) differs from it for e.g. 128 -> 192.
void ingest_index_table(int src, int dst, int *idx)
{
    const double a0 = (double)src / dst;
    double xo = a0 * 0.5;
    for (int x = 0; x < dst; ++x) {
        idx[x] = (int)xo;
        xo += a0;
    }
}

bool ingest_shape_ok(int n, int src_h, int src_w, int H, int W)
{
    // one staged image and one sample of an output are each addressed by 32-bit byte offsets under one buffer resource
    return n >= 1 && n <= 65535 && src_h >= 1 && src_w >= 1 && H >= 32 && W >= 32 && H % 32 == 0 && W % 32 == 0 &&
           3l * src_h * src_w <= kRsrcMaxBytes && 24l * H * W <= kRsrcMaxBytes;
}

void launch_ingest(IngestArgs a, hipStream_t stream)
{
    const bool ident = a.src_h == a.H && a.src_w == a.W;
    const int lanes = a.H * a.W / 4, qlanes = lanes / 16;
    // 256-lane workgroups, or single waves while those would not give every compute unit two workgroups (batch 1 at 192 x 256: 204 waves)
    const int threads = (long)a.N * (lanes / 256) < 512 ? 64 : 256;
    a.full_blocks = lanes / threads;
    const dim3 grid((unsigned)(a.full_blocks + (qlanes + threads - 1) / threads), (unsigned)a.N);
    if (ident) hipLaunchKernelGGL(ingest_kernel<true>, grid, dim3(threads), 0, stream, a);
    else hipLaunchKernelGGL(ingest_kernel<false>, grid, dim3(threads), 0, stream, a);
}

}  // namespace demon
