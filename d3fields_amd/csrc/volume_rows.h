// volume_rows.h -- the per-point pieces of the baked-volume lookups (DESIGN.md sections 13 and 15), shared by the dense samplers
// (volume_kernels.hip: corner rows at voxel * stride) and the band samplers (band_kernels.hip: corner rows at slot[voxel] * stride):
// locating a point, the fill row, the eight-corner chain over a set's channels and its derivative.  ONE definition, so a banded
// lookup and a dense one round alike.  The callers differ only in how they form the eight row pointers.
#pragma once
#include "d3f_internal.h"
#include "volume_cell.h"      // corner_weights, corner_offset, blend

namespace d3f {

constexpr int kNotValid = -1;      // Cell::base of a point outside the volume or in a cell with an invalid corner
constexpr int kNoPoint = -2;       // ... of a lane past the last point

struct Cell {
    int32_t base;                  // flat index of the cell's corner (0,0,0), < nx*ny*nz <= 2^31 - 1
    float tx, ty, tz;
};

// the point (px, py, pz) itself (align_kernels.hip locates transformed points, which live in no array)
// cell: the flat CELL index of a valid point (untouched otherwise)
__device__ __forceinline__ Cell locate_at(const VolParams &P, float px, float py, float pz, int64_t &cell)
{
    const float gx = (px - P.ox) / P.h, gy = (py - P.oy) / P.h, gz = (pz - P.oz) / P.h;
    Cell c;
    c.base = kNotValid;
    c.tx = c.ty = c.tz = 0.0f;
    // (NaN fails every comparison)
    const bool inside = gx >= 0.0f && gx <= (float)(P.nx - 1) && gy >= 0.0f && gy <= (float)(P.ny - 1) && gz >= 0.0f && gz <= (float)(P.nz - 1);
    if (inside) {
        const int ix = min((int)floorf(gx), P.nx - 2), iy = min((int)floorf(gy), P.ny - 2), iz = min((int)floorf(gz), P.nz - 2);
        c.tx = gx - (float)ix;
        c.ty = gy - (float)iy;
        c.tz = gz - (float)iz;
        const int64_t at = ((int64_t)ix * (P.ny - 1) + iy) * (P.nz - 1) + iz;
        if (P.cell[at] != 0) {
            c.base = (ix * P.ny + iy) * P.nz + iz;
            cell = at;
        }
    }
    return c;
}

// point i of P.pts
__device__ __forceinline__ Cell locate(const VolParams &P, int64_t i, int64_t &cell)
{
    const float *p = P.pts + 3 * i;
    return locate_at(P, p[0], p[1], p[2], cell);
}

__device__ __forceinline__ Cell locate(const VolParams &P, int64_t i)
{
    int64_t cell;
    return locate(P, i, cell);
}

__device__ __forceinline__ float4 blend4(const float (&w)[8], const float4 (&v)[8])
{
    float4 acc = make_float4(w[0] * v[0].x, w[0] * v[0].y, w[0] * v[0].z, w[0] * v[0].w);
#pragma unroll
    for (int c = 1; c < 8; ++c) {
        acc.x = fmaf(w[c], v[c].x, acc.x);
        acc.y = fmaf(w[c], v[c].y, acc.y);
        acc.z = fmaf(w[c], v[c].z, acc.z);
        acc.w = fmaf(w[c], v[c].w, acc.w);
    }
    return acc;
}

__device__ __forceinline__ float fill_of(const VolSet &S, int ch) { return S.fill ? S.fill[ch] : 0.0f; }

// ---- rows stored as IEEE half (VolSet::f16; include/d3fields_hip.h) ------------------------------------------
// A stored half is widened to float32 exactly (one v_cvt_f32_f16; subnormals, signed zeros, Inf and NaN keep their value) and then
// takes the float32 chain above unchanged: w0 * v0 is a plain multiply, the seven other corners are fmaf.  One 16-byte load is eight
// channels, so a vector step is two blend4 / eight add_derivative.
// The eight halves of a vector stay four packed words until a channel is needed (kept as integers so that the compiler does not widen
// all eight corners x eight channels up front: 64 VGPRs where the float32 form holds 32).
__device__ __forceinline__ float widen(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }

template <int J>      // channel J = 0..7 of a 16-byte vector of halves
__device__ __forceinline__ float channel_f16(const uint4 &r)
{
    const uint32_t word = J < 2 ? r.x : J < 4 ? r.y : J < 6 ? r.z : r.w;
    return widen((J & 1) ? word >> 16 : word & 0xffffu);
}

// channels FIRST .. FIRST + 3 of eight corner vectors, widened
template <int FIRST>
__device__ __forceinline__ float4 blend4_f16(const float (&w)[8], const uint4 (&r)[8])
{
    float4 v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = make_float4(channel_f16<FIRST>(r[c]), channel_f16<FIRST + 1>(r[c]), channel_f16<FIRST + 2>(r[c]), channel_f16<FIRST + 3>(r[c]));
    return blend4(w, v);
}

// the row loops of sample_row for a half set; o: the output row of the point
template <class Rows>
__device__ __forceinline__ void sample_row_f16(const VolSet &S, float *o, const float (&w)[8], int first, int lanes, Rows rows)
{
    const _Float16 *row[8];
    rows(row);
    if (S.vec) {
        for (int k = 8 * first; k < S.C; k += 8 * lanes) {
            uint4 r[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) r[c] = *reinterpret_cast<const uint4 *>(row[c] + k);
            *reinterpret_cast<float4 *>(o + k) = blend4_f16<0>(w, r);
            __builtin_amdgcn_sched_barrier(0);      // the first four channels are done before the other four are widened
            *reinterpret_cast<float4 *>(o + k + 4) = blend4_f16<4>(w, r);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (float)row[c][k];
            o[k] = blend(w, v);
        }
    }
}

// channels [first, C) in steps of `lanes` vectors / floats of the row of point i: lanes = 1 is phase A, 16 is phase B.
// rows(row): called for a point that has rows (`has`), fills the eight corner row pointers; otherwise the fill row is written
// (float32 in either storage: a half set with vectors has C % 8 == 0 and 16-byte output rows, so the float4 loop covers it).
// F16: the instance may meet half sets (a wave-uniform branch per set, outside the channel loop); false is the float32-only code.
template <bool F16 = false, class Rows>
__device__ __forceinline__ void sample_row(const VolSet &S, int64_t i, bool has, const float (&w)[8], int first, int lanes, Rows rows)
{
    float *o = S.out + i * S.C;
    if (!has) {
        if (S.vec) {
            for (int k = 4 * first; k < S.C; k += 4 * lanes)
                *reinterpret_cast<float4 *>(o + k) = make_float4(fill_of(S, k), fill_of(S, k + 1), fill_of(S, k + 2), fill_of(S, k + 3));
        } else {
            for (int k = first; k < S.C; k += lanes) o[k] = fill_of(S, k);
        }
        return;
    }
    if (F16 && S.f16) {
        sample_row_f16(S, o, w, first, lanes, rows);
        return;
    }
    const float *row[8];
    rows(row);
    if (S.vec) {
        for (int k = 4 * first; k < S.C; k += 4 * lanes) {
            float4 v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(row[c] + k);
            *reinterpret_cast<float4 *>(o + k) = blend4(w, v);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = row[c][k];
            o[k] = blend(w, v);
        }
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
struct FaceWeights {
    float yz[4], xz[4], xy[4];      // products of the two OTHER axes' weights, index = first * 2 + second
};

__device__ __forceinline__ FaceWeights face_weights(float tx, float ty, float tz)
{
    const float ax[2] = {1.0f - tx, tx}, ay[2] = {1.0f - ty, ty}, az[2] = {1.0f - tz, tz};
    FaceWeights f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        f.yz[j] = ay[j >> 1] * az[j & 1];
        f.xz[j] = ax[j >> 1] * az[j & 1];
        f.xy[j] = ax[j >> 1] * ay[j & 1];
    }
    return f;
}

// acc += g * d blend / d (tx, ty, tz) for one channel with corner values v
__device__ __forceinline__ void add_derivative(const FaceWeights &f, const float (&v)[8], float g, float (&acc)[3])
{
    float dx = f.yz[0] * (v[4] - v[0]);
    dx = fmaf(f.yz[1], v[5] - v[1], dx);
    dx = fmaf(f.yz[2], v[6] - v[2], dx);
    dx = fmaf(f.yz[3], v[7] - v[3], dx);
    float dy = f.xz[0] * (v[2] - v[0]);
    dy = fmaf(f.xz[1], v[3] - v[1], dy);
    dy = fmaf(f.xz[2], v[6] - v[4], dy);
    dy = fmaf(f.xz[3], v[7] - v[5], dy);
    float dz = f.xy[0] * (v[1] - v[0]);
    dz = fmaf(f.xy[1], v[3] - v[2], dz);
    dz = fmaf(f.xy[2], v[5] - v[4], dz);
    dz = fmaf(f.xy[3], v[7] - v[6], dz);
    acc[0] = fmaf(g, dx, acc[0]);
    acc[1] = fmaf(g, dy, acc[1]);
    acc[2] = fmaf(g, dz, acc[2]);
}

// acc += g * d blend / d (tx, ty, tz) for channel J of eight corner vectors
template <int J>
__device__ __forceinline__ void add_derivative_f16(const FaceWeights &f, const uint4 (&r)[8], float g, float (&acc)[3])
{
    const float v[8] = {channel_f16<J>(r[0]), channel_f16<J>(r[1]), channel_f16<J>(r[2]), channel_f16<J>(r[3]),
                        channel_f16<J>(r[4]), channel_f16<J>(r[5]), channel_f16<J>(r[6]), channel_f16<J>(r[7])};
    add_derivative(f, v, g, acc);
    __builtin_amdgcn_sched_barrier(0);      // one channel's eight widened corners at a time
}

// the row loops of backward_row for a half set; g: the (float32) gradient row of the point.  Channels are summed in ascending order within
// a lane, eight to a vector step: with one lane (a narrow set) that is the float32 form's order, with sixteen the channel -> lane map differs.
template <class Rows>
__device__ __forceinline__ void backward_row_f16(const VolSet &S, const float *g, const FaceWeights &f, int first, int lanes, float (&acc)[3], Rows rows)
{
    const _Float16 *row[8];
    rows(row);
    if (S.vec) {
        for (int k = 8 * first; k < S.C; k += 8 * lanes) {
            uint4 r[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) r[c] = *reinterpret_cast<const uint4 *>(row[c] + k);
            const float4 g0 = *reinterpret_cast<const float4 *>(g + k), g1 = *reinterpret_cast<const float4 *>(g + k + 4);
            add_derivative_f16<0>(f, r, g0.x, acc);
            add_derivative_f16<1>(f, r, g0.y, acc);
            add_derivative_f16<2>(f, r, g0.z, acc);
            add_derivative_f16<3>(f, r, g0.w, acc);
            add_derivative_f16<4>(f, r, g1.x, acc);
            add_derivative_f16<5>(f, r, g1.y, acc);
            add_derivative_f16<6>(f, r, g1.z, acc);
            add_derivative_f16<7>(f, r, g1.w, acc);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = (float)row[c][k];
            add_derivative(f, v, g[k], acc);
        }
    }
}

// S.grad is not null; rows(row) fills the eight corner row pointers of the point's cell.  F16: as sample_row
template <bool F16 = false, class Rows>
__device__ __forceinline__ void backward_row(const VolSet &S, int64_t i, const FaceWeights &f, int first, int lanes, float (&acc)[3], Rows rows)
{
    const float *g = S.grad + i * S.C;
    if (F16 && S.f16) {
        backward_row_f16(S, g, f, first, lanes, acc, rows);
        return;
    }
    const float *row[8];
    rows(row);
    if (S.vec) {
        for (int k = 4 * first; k < S.C; k += 4 * lanes) {
            float4 v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = *reinterpret_cast<const float4 *>(row[c] + k);
            const float4 gk = *reinterpret_cast<const float4 *>(g + k);
            const float a[8] = {v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x};
            const float b[8] = {v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y};
            const float c2[8] = {v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z};
            const float d[8] = {v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w};
            add_derivative(f, a, gk.x, acc);
            add_derivative(f, b, gk.y, acc);
            add_derivative(f, c2, gk.z, acc);
            add_derivative(f, d, gk.w, acc);
        }
    } else {
        for (int k = first; k < S.C; k += lanes) {
            float v[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] = row[c][k];
            add_derivative(f, v, g[k], acc);
        }
    }
}

}  // namespace d3f
