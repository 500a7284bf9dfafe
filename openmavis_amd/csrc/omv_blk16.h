// Where entry (r, c) of a stored 16x16 block sits: one text for the kernels that write and factor the blocks
// (omv_ldlt.h, lba.hip, essgraph.hip) and the host code that reads them back (omv_ldlt_host.h, also under g++).
#pragma once
#ifdef __HIPCC__
#define OMV_HD __host__ __device__
#else
#define OMV_HD
#endif

// Entry (r, c) of a 16x16 block sits at 16 r + (c ^ r): a column read by 16 lanes (one per row), as the MFMA
// A operands and the pivot columns are, touches 16 distinct LDS banks instead of two (rows are 32 banks apart).
OMV_HD inline int sw16(int r, int c) { return 16 * r + (c ^ r); }
