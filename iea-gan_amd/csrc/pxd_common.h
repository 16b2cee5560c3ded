// Launch partition shared by the kernels that walk a batch of PXD sensor images (pxd_stats.hip, pxd_digits.hip):
// grid (P, N), workgroup (p, n) owns a contiguous pixel range of image n.
#pragma once

#define PXD_THREADS 256
#define PXD_CHUNK 4096          // pixels per block at the least: 4 float4 / 1 x 16 uint8 per thread
#define PXD_MAX_BLOCKS 2048
#define PXD_MAX_PARTS 64

static inline int pxd_parts(int N, long HW) {
    long p = (HW + PXD_CHUNK - 1) / PXD_CHUNK;
    const long cap = PXD_MAX_BLOCKS / N > 1 ? PXD_MAX_BLOCKS / N : 1;
    if (p > cap) p = cap;
    if (p > PXD_MAX_PARTS) p = PXD_MAX_PARTS;
    return (int)(p < 1 ? 1 : p);
}
