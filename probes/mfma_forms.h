// The matrix-core forms that more than one probe kernel issues, each stated
// once, for the tile kernels and the unit sweep alike. A form is a struct of
// static members:
//   Acc, REGS          the lane's accumulator type and register count
//   In, Frag           the row-major operands in memory; the lane's operand
//                      registers (`a` is the A operand)
//   load(In, lane)     the operand lane map
//   mma(Frag, Acc)     the builtin, with its format immediates
//   d_index(lane, reg) the result map: row-major index of register `reg`
// form_tile<Form>, at the end, is the body of every tile kernel on a form.
// Forms that a single kernel uses (f64, i8, 2:4 sparse) stay in that kernel.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

namespace {

constexpr int MFMA_LANES = 64;  // one wave (gfx950); a tile has REGS × 64 elements

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x16 __attribute__((ext_vector_type(16)));

// C/D of every 16×16 form but f64 (cdna_hip_programming.md §3).
__device__ constexpr int d_index_16x16(int l, int reg) {
    return (4 * (l >> 4) + reg) * 16 + (l & 15);
}

// C/D of every 32×32 form (cdna_hip_programming.md §3).
__device__ constexpr int d_index_32x32(int l, int reg) {
    return ((reg & 3) + 8 * (reg >> 2) + 4 * (l >> 5)) * 32 + (l & 31);
}

// v_mfma_f32_16x16x4_f32. Lane mapping from cdna_hip_programming.md §3
// (documented, exact f32): a = A[l&15][l>>4] (K=4: k = l>>4), b = B[l>>4][l&15].
struct MfmaF32x16x16x4 {
    using Acc = f32x4;
    static constexpr int REGS = 4;
    struct In { const float *A, *B; };  // 16×4 and 4×16
    struct Frag { float a, b; };
    static __device__ __forceinline__ Frag load(const In& in, int l) {
        int rc = l & 15, k = l >> 4;
        return {in.A[rc * 4 + k], in.B[k * 16 + rc]};
    }
    static __device__ __forceinline__ Acc mma(const Frag& f, Acc acc) {
        return __builtin_amdgcn_mfma_f32_16x16x4f32(f.a, f.b, acc, 0, 0, 0);
    }
    static __device__ constexpr int d_index(int l, int reg) { return d_index_16x16(l, reg); }
};

// v_mfma_f32_32x32x16_bf16 / _f16 (T = __bf16 or _Float16; same maps and
// cycles): each lane holds 8 elements of A and of B (4 VGPRs each) and 16 f32
// accumulators. A/B input mapping (K=16, 2 lane-halves of 32): lane l holds
//   A[l&31][(l>>5)*8 + j]  and  B[(l>>5)*8 + j][l&31],  j = 0..7.
// The numeric check against a host reference catches any mapping error.
template <class T>
struct Mfma32x32x16 {
    static_assert(std::is_same_v<T, __bf16> || std::is_same_v<T, _Float16>, "bf16 or f16");
    using Acc = f32x16;
    static constexpr int REGS = 16;
    typedef T Vec8 __attribute__((ext_vector_type(8)));
    struct In { const T *A, *B; };  // 32×16 and 16×32
    struct Frag { Vec8 a, b; };
    static __device__ __forceinline__ Frag load(const In& in, int l) {
        int half = l >> 5, lane32 = l & 31;  // half: which 8-wide K slice
        Frag f;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            f.a[j] = in.A[lane32 * 16 + half * 8 + j];
            f.b[j] = in.B[(half * 8 + j) * 32 + lane32];
        }
        return f;
    }
    static __device__ __forceinline__ Acc mma(const Frag& f, Acc acc) {
        if constexpr (std::is_same_v<T, __bf16>)
            return __builtin_amdgcn_mfma_f32_32x32x16_bf16(f.a, f.b, acc, 0, 0, 0);
        else
            return __builtin_amdgcn_mfma_f32_32x32x16_f16(f.a, f.b, acc, 0, 0, 0);
    }
    static __device__ constexpr int d_index(int l, int reg) { return d_index_32x32(l, reg); }
};

// FP8 and block-scaled MX (FP8/FP4) MFMA. Operands arrive as row-major element
// codes, one uint8 per element; load() does the lane packing, so the lane
// maps below are the ones tests/test_gpu_lowp_kernels.py pins on hardware
// (decode sweep, one-k-at-a-time identity, scale map).
// Format numbers are the instruction's own cbsz (A) / blgp (B) encodings.
// FP6 (e2m3 = 2, e3m2 = 3) needs 6-bit packing and runs at the FP4 rate on
// the same datapath; it is out of scope here.
constexpr int FMT_E4M3 = 0, FMT_E5M2 = 1, FMT_E2M1 = 4;

// v_mfma_f32_16x16x32_{fp8,bf8}_{fp8,bf8}: lane l holds A[l&15][8(l>>4)+j]
// and B[8(l>>4)+j][l&15] in byte j of its 64-bit operand.
template <int AF, int BF>
struct MfmaFp8x16x16x32 {
    using Acc = f32x4;
    static constexpr int REGS = 4;
    struct In { const uint8_t *A, *B; };  // 16×32 and 32×16 codes
    struct Frag { uint64_t a, b; };
    static __device__ __forceinline__ Frag load(const In& in, int l) {
        int rc = l & 15, g = l >> 4;
        Frag f = {0, 0};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            f.a |= (uint64_t)in.A[rc * 32 + 8 * g + j] << (8 * j);
            f.b |= (uint64_t)in.B[(8 * g + j) * 16 + rc] << (8 * j);
        }
        return f;
    }
    static __device__ __forceinline__ Acc mma(const Frag& f, Acc acc) {
        if constexpr (AF == FMT_E4M3 && BF == FMT_E4M3)
            return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8((long)f.a, (long)f.b, acc, 0, 0, 0);
        else if constexpr (AF == FMT_E4M3)
            return __builtin_amdgcn_mfma_f32_16x16x32_fp8_bf8((long)f.a, (long)f.b, acc, 0, 0, 0);
        else if constexpr (BF == FMT_E4M3)
            return __builtin_amdgcn_mfma_f32_16x16x32_bf8_fp8((long)f.a, (long)f.b, acc, 0, 0, 0);
        else
            return __builtin_amdgcn_mfma_f32_16x16x32_bf8_bf8((long)f.a, (long)f.b, acc, 0, 0, 0);
    }
    static __device__ constexpr int d_index(int l, int reg) { return d_index_16x16(l, reg); }
};

// v_mfma_scale_f32_16x16x128_f8f6f4 operand maps, as the tests established
// them on an MI355X (they differ by format, and from the bf16-style guess):
//   * lane l works on row (A) or column (B) l&15; g = l>>4.
//   * fp4: 4 dwords, two elements per byte, the even one in the low nibble;
//     element e = 0..31 of lane group g is k = 32g + e.
//   * fp8: 8 dwords, element e in byte e; e = 0..15 is k = 16g + e and
//     e = 16..31 is k = 64 + 16g + (e-16): a lane holds two 16-wide runs,
//     64 apart, not one 32-wide block.
//   * byte 0 of the scale VGPR (op_sel 0) of lane (l&15, g) is the E8M0 scale
//     of k = 32g .. 32g+31 of that row or column — for fp4 the lane's own
//     elements, for fp8 elements held by other lanes.
// With these, D[i][j] = Σ_b 2^(sa[i][b]-127)·2^(sb[b][j]-127)·Σ_{k∈32b..32b+31} a·b
// for every format pair, mixed ones included.
template <int FMT>
__device__ constexpr int mx_k(int g, int e) {
    return FMT == FMT_E2M1 ? 32 * g + e : 64 * (e >> 4) + 16 * g + (e & 15);
}

// One lane's 32 element codes, in element order, → its operand registers
// (fp4 fills the first four dwords; the other four are not read).
template <int FMT>
__device__ i32x8 pack_mx(const uint8_t (&code)[32]) {
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 32; e++) {
        if constexpr (FMT == FMT_E2M1) w[e >> 3] |= (code[e] & 15u) << (4 * (e & 7));
        else w[e >> 2] |= (uint32_t)code[e] << (8 * (e & 3));
    }
    i32x8 v;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = (int)w[i];
    return v;
}

template <int AF, int BF>
struct MfmaMx16x16x128 {
    using Acc = f32x4;
    static constexpr int REGS = 4;
    struct In { const uint8_t *A, *B, *SA, *SB; };  // 16×128, 128×16 codes; 16×4, 4×16 E8M0
    struct Frag { i32x8 a, b; int sa, sb; };
    static __device__ __forceinline__ Frag load(const In& in, int l) {
        int rc = l & 15, g = l >> 4;
        uint8_t ca[32], cb[32];
#pragma unroll
        for (int e = 0; e < 32; e++) {
            ca[e] = in.A[rc * 128 + mx_k<AF>(g, e)];
            cb[e] = in.B[mx_k<BF>(g, e) * 16 + rc];
        }
        return {pack_mx<AF>(ca), pack_mx<BF>(cb), in.SA[rc * 4 + g], in.SB[g * 16 + rc]};
    }
    static __device__ __forceinline__ Acc mma(const Frag& f, Acc acc) {
        return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(f.a, f.b, acc, AF, BF, 0, f.sa,
                                                               0, f.sb);
    }
    static __device__ constexpr int d_index(int l, int reg) { return d_index_16x16(l, reg); }
};

// The body of a tile kernel: every block computes the same tile, D = A·B (+ C
// where C is not null), and its first wave stores the block's own slab of
// REGS × 64 floats, so a launch of 2×CUs blocks puts the tile through the
// matrix cores of every CU and the host can compare the slabs.
template <class Form>
__device__ __forceinline__ void form_tile(const typename Form::In& in, const float* C,
                                          float* D) {
    int l = threadIdx.x & (MFMA_LANES - 1);
    typename Form::Frag f = Form::load(in, l);
    typename Form::Acc acc = {};
    if (C) {
        for (int reg = 0; reg < Form::REGS; reg++) acc[reg] = C[Form::d_index(l, reg)];
    }
    acc = Form::mma(f, acc);
    if (threadIdx.x < MFMA_LANES) {
        float* slab = D + (size_t)blockIdx.x * (Form::REGS * MFMA_LANES);
        for (int reg = 0; reg < Form::REGS; reg++) slab[Form::d_index(l, reg)] = acc[reg];
    }
}

}  // namespace
