// viewgeom.h -- declarations of viewgeom.hip (view tools: visibility masks, depth ratios, consistency counts).  They are kept out of
// internal.h on purpose: internal.h is part of the kernel-source hash that stamps the network's profiles and its recorded dispatch
// trace (demon_amd/build.py csrc_sha), and the view tools are not on the network's path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace demon {

constexpr int kViewChunk = 1024;    // pixels of view 1 per workgroup: 256 lanes x 4 consecutive pixels
constexpr int kViewRecord = 40;     // floats per pair record (view_pack_record)
// record layout (float32 unless noted):
//   0 fx  1 cx  2 fy  3 cy | 4..12 R1 transposed, row-major | 13..15 t1 | 16..27 P2 row-major [3][4]
//   28 (float)borderx  29 (float)bordery  30 (float)(width2 - borderx)  31 (float)(height2 - bordery) | 32 (float)W2  33 (float)H2
//   34 lo  35 hi | 36 plane of view 1 (int32 bits)  37 plane of view 2 (int32 bits) | 38, 39 unused (0)
struct ViewArgs {
    const float *depth1;          // planes of h w floats, plane1_stride apart; the record's first index selects one
    const float *depth2;          // planes of H2 W2 floats, plane2_stride apart, or null: no ratios (mask and valid1 only)
    const float *records;         // [n][kViewRecord]
    uint8_t *mask;                // [n][h w], or null (only read by the instances that store it)
    float *ratios;                // [n][h w], or null
    int *chunk_counts;            // workspace [n][chunks][4]
    int *counts;                  // [n][4]: valid1, visible, ratios, consistent
    long plane1_stride, plane2_stride;
    int n, h, w;                  // pairs; view 1
    int H2, W2;                   // view 2 (the lookup's clamp and row length)
    int hw, chunks;               // set by the launcher
};
bool view_shape_ok(int h, int w, int H2, int W2);
int view_chunks(int h, int w);
// K1, R1 [3][3], t1 [3], P2 [3][4] (all float32, as view_tools_cython.pyx receives them) -> one record
void view_pack_record(const float *K1, const float *R1, const float *t1, const float *P2, int width2, int height2, int borderx, int bordery,
                      float lo, float hi, int plane1, int plane2, float *out);
// two launches: view_pairs_kernel<mask != null, ratios != null>, then view_counts_kernel
void launch_view_pairs(ViewArgs a, hipStream_t stream);

}  // namespace demon
