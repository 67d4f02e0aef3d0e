// kata_xpu_device_plugin_amd._gpuprobe_formats — MI355X (gfx950) matrix-core
// probes for the formats _gpuprobe does not issue:
//
//   * FP64   v_mfma_f64_16x16x4_f64   — the HPC datapath, with its own C/D
//     register layout (row = (l>>4) + 4·reg, not 4·(l>>4) + reg).
//   * FP16   v_mfma_f32_32x32x16_f16  — the f16 multiplier inputs (the bf16
//     tile's maps and cycles).
//   * INT8   v_mfma_i32_16x16x64_i8   — the integer inference path, i32
//     accumulators, twice the bf16 rate per clock.
//   * 2:4 structured sparsity  v_smfmac_f32_16x16x64_f16 — the per-lane index
//     and select logic that nothing dense exercises.
//
// Each form has a tile kernel (one wave per block, every block the same tile
// into its own slab) behind a raw *_tile_run entry point, FP64 and INT8 have a
// throughput burn, and mfma_probe_formats runs one fixed exact tile per form
// on 2 blocks per CU (slab 0 bitwise against a host product, every slab
// bitwise against slab 0) and then the two timed burns.
//
// Operands arrive row-major and the kernels do the lane packing, so the lane
// maps below (f64, i8, sparse) and in mfma_forms.h (f16, and the 16×16 result
// map) are the ones tests/test_gpu_formats_kernels.py pins on hardware.
//
// Wavefront size is 64 (gfx950). Build: hipcc --offload-arch=gfx950, driven by
// setup.build_hip() next to xpu_probe.hip.

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mfma_forms.h"
#include "probe_host.h"

namespace {

// ---------------------------------------------------------------------------
// v_mfma_f64_16x16x4_f64: one f64 of A and B per lane, as the f32 16x16x4
// form (A[l&15][l>>4], B[l>>4][l&15]); four f64 results per lane with
//   D reg r ↔ D[(l>>4) + 4r][l&15]
// (cdna_hip_programming.md §3: the f64 map, not the 4(l>>4)+r of every other
// 16×16 form).
// ---------------------------------------------------------------------------
__global__ void mfma_f64_tile(const double* __restrict__ A,  // 16×4 row-major
                              const double* __restrict__ B,  // 4×16 row-major
                              const double* __restrict__ C,  // 16×16 or nullptr (= 0)
                              double* __restrict__ D) {      // gridDim.x × 16×16
    int l = threadIdx.x & (WAVE - 1);
    int rc = l & 15, k = l >> 4;
    double a = A[rc * 4 + k];
    double b = B[k * 16 + rc];
    f64x4 acc = {0., 0., 0., 0.};
    if (C) {
        for (int r = 0; r < 4; r++) acc[r] = C[(k + 4 * r) * 16 + rc];
    }
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    if (threadIdx.x < WAVE) {
        double* slab = D + (size_t)blockIdx.x * 256;
        for (int r = 0; r < 4; r++) slab[(k + 4 * r) * 16 + rc] = acc[r];
    }
}

// ---------------------------------------------------------------------------
// v_mfma_f32_32x32x16_f16: the bf16 tile's form with the f16 builtin
// (Mfma32x32x16 in mfma_forms.h).
// ---------------------------------------------------------------------------
__global__ void mfma_f16_tile(const _Float16* __restrict__ A,  // 32×16 row-major
                              const _Float16* __restrict__ B,  // 16×32 row-major
                              float* __restrict__ D) {         // gridDim.x × 32×32
    form_tile<Mfma32x32x16<_Float16>>({A, B}, nullptr, D);
}

// ---------------------------------------------------------------------------
// v_mfma_i32_16x16x64_i8: lane l (rc = l&15, g = l>>4) holds 16 int8 of A and
// of B in its four dwords, byte j = k 16g + j: A[rc][16g+j] and B[16g+j][rc].
// A and B use the same k order, so the product alone cannot tell this map from
// another bijection of (g, j) onto k; the one-k-at-a-time test shows that the
// map is consistent between the operands, which is all a caller relies on.
// C/D as every other 16×16 form (col = l&15, row = 4(l>>4)+reg), i32.
// ---------------------------------------------------------------------------
__device__ constexpr int i8_k(int g, int j) { return 16 * g + j; }

__device__ __forceinline__ i32x4 pack_i8(const int8_t (&v)[16]) {
    uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 16; j++) w[j >> 2] |= (uint32_t)(uint8_t)v[j] << (8 * (j & 3));
    i32x4 r;
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = (int)w[i];
    return r;
}

__global__ void mfma_i8_tile(const int8_t* __restrict__ A,   // 16×64 row-major
                             const int8_t* __restrict__ B,   // 64×16 row-major
                             const int32_t* __restrict__ C,  // 16×16 or nullptr (= 0)
                             int32_t* __restrict__ D) {      // gridDim.x × 16×16
    int l = threadIdx.x & (WAVE - 1);
    int rc = l & 15, g = l >> 4;
    int8_t va[16], vb[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        va[j] = A[rc * 64 + i8_k(g, j)];
        vb[j] = B[i8_k(g, j) * 16 + rc];
    }
    i32x4 a = pack_i8(va), b = pack_i8(vb);
    i32x4 acc = {0, 0, 0, 0};
    if (C) {
        for (int r = 0; r < 4; r++) acc[r] = C[d_index_16x16(l, r)];
    }
    acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc, 0, 0, 0);
    if (threadIdx.x < WAVE) {
        int32_t* slab = D + (size_t)blockIdx.x * 256;
        for (int r = 0; r < 4; r++) slab[d_index_16x16(l, r)] = acc[r];
    }
}

// ---------------------------------------------------------------------------
// v_smfmac_f32_16x16x64_f16: D += A·B where A (16×64) is 2:4 sparse: of every
// four consecutive k, two elements are kept. A arrives as its kept half
// (16×32) plus, per kept element, its position 0..3 in its group of four:
//   D[i][j] = Σ_e A[i][e] · B[4(e>>1) + idx[i][e]][j]
// Lane l (rc = l&15, q = l>>4) holds kept elements 8q..8q+7 of row rc (dense
// k = 16q..16q+15) and in bits 2t..2t+1 of the index register the position of
// kept element 8q+t (cbsz = abid = 0: index bits 15:0). The B lane does not
// hold one 16-wide run, as the CDNA3 16x16x32 description scaled up would
// suggest: as the tests established on an MI355X, element j of lane (rc, q)
// is B[32(j>>3) + 8q + (j&7)][rc] — two 8-wide runs, 32 apart (the K=32
// half-tile's map twice, like the MX-fp8 operand's two runs).
// C/D as every other 16×16 form.
// ---------------------------------------------------------------------------
__device__ constexpr int smfmac_b_k(int q, int j) { return 32 * (j >> 3) + 8 * q + (j & 7); }

__global__ void smfmac_f16_tile(const _Float16* __restrict__ A,   // 16×32 kept values
                                const uint8_t* __restrict__ IDX,  // 16×32, each 0..3
                                const _Float16* __restrict__ B,   // 64×16 row-major
                                float* __restrict__ D) {          // gridDim.x × 16×16
    int l = threadIdx.x & (WAVE - 1);
    int rc = l & 15, q = l >> 4;
    f16x8 a;
    uint32_t idx = 0;
    for (int t = 0; t < 8; t++) {
        a[t] = A[rc * 32 + 8 * q + t];
        idx |= (uint32_t)(IDX[rc * 32 + 8 * q + t] & 3u) << (2 * t);
    }
    f16x16 b;
    for (int j = 0; j < 16; j++) b[j] = B[smfmac_b_k(q, j) * 16 + rc];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_smfmac_f32_16x16x64_f16(a, b, acc, (int)idx, 0, 0);
    if (threadIdx.x < WAVE) {
        float* slab = D + (size_t)blockIdx.x * 256;
        for (int r = 0; r < 4; r++) slab[d_index_16x16(l, r)] = acc[r];
    }
}

// ---------------------------------------------------------------------------
// Throughput burns on the instructions the tile tests verified, in the burns'
// launcher shape (`blocks` × 256 threads, one 4-byte word per lane).
//
// Operands are small integers derived from the lane and element index, so the
// operand map matters and every partial sum is an exact integer:
//   f64: lane l holds A[l&15][l>>4] = 1 + l%3 and B[l>>4][l&15] = 1 + (l^(l>>3))%3;
//   i8:  element j of lane l (k = 16(l>>4)+j of row or column l&15) is
//        1 + (l+j)%3 for A and 1 + (l^j)%3 for B.
// Accumulator n starts at n in every element, which keeps the chains distinct
// for the compiler. One f64 MFMA adds at most 4·9 = 36 to an element and one
// i8 MFMA at most 64·9 = 576. The f64 lane sum (at most 112 + 32·36·iters) is
// stored as f32 and is exact for iters ≤ 14563; the i8 lane sum is stored as
// its i32 bits. Longer burns round (f64→f32) or wrap, identically in every
// wave.
//
// Eight independent accumulators per wave and two waves per SIMD, as the MX
// burn: the dependent-accumulator latency of neither form is documented. The
// i8 form takes the cycles of bf16 16x16x32 (16 per issue at the bf16 rate),
// so eight chains put 128 cycles between dependent issues; the f64 form runs
// at a fraction of the f32 rate (≥32 cycles per issue), so eight chains put
// ≥256 cycles between them. Either covers any plausible latency (the f32
// 16x16x4 form's is 40), at 64 (f64) and 32 (i8) accumulator registers.
// Measured on MI355X: ≈76 TF f64 (half the f32 16x16x4 rate, so 64 cycles per
// issue) and ≈4500 TOPS i8, 90 % of 2× bf16 (profiles/mfma_formats.md).
// ---------------------------------------------------------------------------
constexpr int FMT_BURN_ACCS = 8;

__global__ void __launch_bounds__(256, 2)
mfma_f64_burn(float* __restrict__ out, int iters) {
    int l = threadIdx.x & (WAVE - 1);
    double a = (double)(1 + l % 3);
    double b = (double)(1 + (l ^ (l >> 3)) % 3);
    f64x4 acc[FMT_BURN_ACCS];
#pragma unroll
    for (int n = 0; n < FMT_BURN_ACCS; n++)
        acc[n] = {(double)n, (double)n, (double)n, (double)n};
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int n = 0; n < FMT_BURN_ACCS; n++)
            acc[n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc[n], 0, 0, 0);
    }
    double s = 0;
#pragma unroll
    for (int n = 0; n < FMT_BURN_ACCS; n++) s += acc[n][0] + acc[n][1] + acc[n][2] + acc[n][3];
    // one store per lane
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = (float)s;
}

__global__ void __launch_bounds__(256, 2)
mfma_i8_burn(float* __restrict__ out, int iters) {
    int l = threadIdx.x & (WAVE - 1);
    int8_t va[16], vb[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        va[j] = (int8_t)(1 + (l + j) % 3);
        vb[j] = (int8_t)(1 + (l ^ j) % 3);
    }
    i32x4 a = pack_i8(va), b = pack_i8(vb);
    i32x4 acc[FMT_BURN_ACCS];
#pragma unroll
    for (int n = 0; n < FMT_BURN_ACCS; n++) acc[n] = {n, n, n, n};
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int n = 0; n < FMT_BURN_ACCS; n++)
            acc[n] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, acc[n], 0, 0, 0);
    }
    uint32_t s = 0;   // unsigned: the sum wraps instead of overflowing
#pragma unroll
    for (int n = 0; n < FMT_BURN_ACCS; n++)
        s += (uint32_t)acc[n][0] + (uint32_t)acc[n][1] + (uint32_t)acc[n][2] +
             (uint32_t)acc[n][3];
    // one store per lane: the i32 sum's bits in the launcher shape's f32 word
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = __uint_as_float(s);
}

// ---------------------------------------------------------------------------
// Host-side wrappers
// ---------------------------------------------------------------------------

// The tile launches fetch through launch_fetch, which moves 4-byte words: an
// f64 slab is 512 of them, an i32 slab 256, compared and returned as bytes.

// One launch of mfma_f64_tile on `blocks` blocks → blocks × 512 words
// (256 f64). C may be nullptr (zero accumulator).
std::vector<float> run_f64_tile(const double* A, const double* B, const double* C,
                                int blocks) {
    DevBuf dA = upload(A, 64 * 8), dB = upload(B, 64 * 8), dC(256 * 8);
    if (C) HIP_CHECK(hipMemcpy(dC.p, C, 256 * 8, hipMemcpyHostToDevice));
    return launch_fetch((size_t)blocks * 512, [&](float* dD) {
        hipLaunchKernelGGL(mfma_f64_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<double>(), dB.as<double>(),
                           C ? dC.as<double>() : (const double*)nullptr,
                           reinterpret_cast<double*>(dD));
    });
}

// One launch of mfma_f16_tile on `blocks` blocks → blocks × 1024 floats.
std::vector<float> run_f16_tile(const uint16_t* A, const uint16_t* B, int blocks) {
    DevBuf dA = upload(A, 512 * 2), dB = upload(B, 512 * 2);
    return launch_fetch((size_t)blocks * 1024, [&](float* dD) {
        hipLaunchKernelGGL(mfma_f16_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const _Float16>(), dB.as<const _Float16>(), dD);
    });
}

// One launch of mfma_i8_tile on `blocks` blocks → blocks × 256 words (i32).
std::vector<float> run_i8_tile(const int8_t* A, const int8_t* B, const int32_t* C,
                               int blocks) {
    DevBuf dA = upload(A, 1024), dB = upload(B, 1024), dC(256 * 4);
    if (C) HIP_CHECK(hipMemcpy(dC.p, C, 256 * 4, hipMemcpyHostToDevice));
    return launch_fetch((size_t)blocks * 256, [&](float* dD) {
        hipLaunchKernelGGL(mfma_i8_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const int8_t>(), dB.as<const int8_t>(),
                           C ? dC.as<const int32_t>() : (const int32_t*)nullptr,
                           reinterpret_cast<int32_t*>(dD));
    });
}

// One launch of smfmac_f16_tile on `blocks` blocks → blocks × 256 floats.
std::vector<float> run_smfmac_tile(const uint16_t* A, const uint8_t* idx,
                                   const uint16_t* B, int blocks) {
    DevBuf dA = upload(A, 512 * 2), dI = upload(idx, 512), dB = upload(B, 1024 * 2);
    return launch_fetch((size_t)blocks * 256, [&](float* dD) {
        hipLaunchKernelGGL(smfmac_f16_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const _Float16>(), dI.as<const uint8_t>(),
                           dB.as<const _Float16>(), dD);
    });
}

py::bytes mfma_f64_tile_run(int dev, py::buffer A, py::buffer B, py::object C, int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A.request(), ib = B.request();
    const double* pa = typed_buffer<double>(ia, 64, "A must be 16x4 contiguous f64");
    const double* pb = typed_buffer<double>(ib, 64, "B must be 4x16 contiguous f64");
    py::buffer_info ic;
    const double* pc = nullptr;
    if (!C.is_none()) {
        require(py::isinstance<py::buffer>(C), "C must be 16x16 contiguous f64");
        ic = py::cast<py::buffer>(C).request();
        pc = typed_buffer<double>(ic, 256, "C must be 16x16 contiguous f64");
    }
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_f64_tile(pa, pb, pc, blocks));
}

py::bytes mfma_f16_tile_run(int dev, py::buffer A_bits, py::buffer B_bits, int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A_bits.request(), ib = B_bits.request();
    const uint16_t* pa = typed_buffer<uint16_t>(ia, 512, "A_bits must be 32x16 contiguous uint16");
    const uint16_t* pb = typed_buffer<uint16_t>(ib, 512, "B_bits must be 16x32 contiguous uint16");
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_f16_tile(pa, pb, blocks));
}

py::bytes mfma_i8_tile_run(int dev, py::buffer A, py::buffer B, py::object C, int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A.request(), ib = B.request();
    const int8_t* pa = typed_buffer<int8_t>(ia, 1024, "A must be 16x64 contiguous int8");
    const int8_t* pb = typed_buffer<int8_t>(ib, 1024, "B must be 64x16 contiguous int8");
    py::buffer_info ic;
    const int32_t* pc = nullptr;
    if (!C.is_none()) {
        require(py::isinstance<py::buffer>(C), "C must be 16x16 contiguous int32");
        ic = py::cast<py::buffer>(C).request();
        pc = typed_buffer<int32_t>(ic, 256, "C must be 16x16 contiguous int32");
    }
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_i8_tile(pa, pb, pc, blocks));
}

py::bytes smfmac_f16_tile_run(int dev, py::buffer A_bits, py::buffer A_idx,
                              py::buffer B_bits, int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A_bits.request(), ii = A_idx.request(), ib = B_bits.request();
    const uint16_t* pa = typed_buffer<uint16_t>(ia, 512, "A_bits must be 16x32 contiguous uint16");
    const uint8_t* pi = typed_buffer<uint8_t>(ii, 512, "A_idx must be 16x32 contiguous uint8");
    const uint16_t* pb = typed_buffer<uint16_t>(ib, 1024, "B_bits must be 64x16 contiguous uint16");
    for (int i = 0; i < 512; i++) require(pi[i] <= 3, "A_idx: an index must be in 0..3");
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_smfmac_tile(pa, pi, pb, blocks));
}

void launch_f64_burn(int blocks, float* out, int iters) {
    hipLaunchKernelGGL(mfma_f64_burn, dim3(blocks), dim3(256), 0, 0, out, iters);
}

void launch_i8_burn(int blocks, float* out, int iters) {
    hipLaunchKernelGGL(mfma_i8_burn, dim3(blocks), dim3(256), 0, 0, out, iters);
}

py::dict mfma_f64_burn_run(int dev, int iters, int blocks) {
    require_dev(dev);
    require(iters > 0, "iters must be > 0");
    require_burn_blocks(blocks);
    HIP_CHECK(hipSetDevice(dev));
    return raw_burn(launch_f64_burn, burn_blocks(dev, blocks, 2), iters);
}

py::dict mfma_i8_burn_run(int dev, int iters, int blocks) {
    require_dev(dev);
    require(iters > 0, "iters must be > 0");
    require_burn_blocks(blocks);
    HIP_CHECK(hipSetDevice(dev));
    return raw_burn(launch_i8_burn, burn_blocks(dev, blocks, 2), iters);
}

// --- probe inputs --------------------------------------------------------------

// A random integer in -range..range.
int lcg_int(uint64_t& s, int range) { return (int)(lcg_bits(s) % (2 * range + 1)) - range; }

// The f16 bit pattern of an integer of magnitude below 2048 (exact in f16).
uint16_t f16_bits_of_int(int v) {
    uint16_t sign = v < 0 ? 0x8000 : 0;
    uint32_t m = (uint32_t)std::abs(v);
    if (m == 0) return sign;
    int e = 0;
    while ((m >> (e + 1)) != 0) e++;          // m in [2^e, 2^(e+1)), e ≤ 10
    uint32_t frac = (m << (10 - e)) & 0x3ff;
    return (uint16_t)(sign | (uint32_t)(e + 15) << 10 | frac);
}

// f64 exact tile: A and B are integers below 2^24 in magnitude times 2^-1 or
// 2^0, so a product is a multiple of the step 2^-2 and below 2^48 = 2^50
// steps; C is such an integer times 2^22, below 2^46. Four products plus C
// stay below 2^53 steps, so every partial sum is exact in f64 in any order,
// fused or not, and the comparison is bitwise.
TileVerdict f64_exact_tile(int blocks) {
    uint64_t rng = 0xBE5466CF34E90C6Cull;
    std::vector<double> A(64), B(64), C(256), ref(256);
    auto draw = [&] {
        int n = lcg_int(rng, (1 << 24) - 1);
        return std::ldexp((double)n, -(int)(lcg_bits(rng) & 1));
    };
    for (double& v : A) v = draw();
    for (double& v : B) v = draw();
    for (double& v : C) v = std::ldexp((double)lcg_int(rng, (1 << 24) - 1), 22);
    for (int i = 0; i < 16; i++)
        for (int j = 0; j < 16; j++) {
            double s = C[i * 16 + j];
            for (int k = 0; k < 4; k++) s += A[i * 4 + k] * B[k * 16 + j];
            ref[i * 16 + j] = s;
        }
    return judge_tile(run_f64_tile(A.data(), B.data(), C.data(), blocks), ref);
}

// f16 exact tile: integer-valued f16 in -16..16. A product is at most 256 and
// 16 of them sum to at most 4096: every partial sum is an integer below 2^24.
TileVerdict f16_exact_tile(int blocks) {
    uint64_t rng = 0xC0AC29B7C97C50DDull;
    std::vector<int> a(512), b(512);
    std::vector<uint16_t> A(512), B(512);
    for (int i = 0; i < 512; i++) A[i] = f16_bits_of_int(a[i] = lcg_int(rng, 16));
    for (int i = 0; i < 512; i++) B[i] = f16_bits_of_int(b[i] = lcg_int(rng, 16));
    std::vector<float> ref(1024);
    for (int i = 0; i < 32; i++)
        for (int j = 0; j < 32; j++) {
            int s = 0;
            for (int k = 0; k < 16; k++) s += a[i * 16 + k] * b[k * 32 + j];
            ref[i * 32 + j] = (float)s;
        }
    return judge_tile(run_f16_tile(A.data(), B.data(), blocks), ref);
}

// i8 exact tile: full-range int8 and a C of up to ±2^30; |Σ| ≤ 64·2^14 = 2^20,
// so nothing wraps.
TileVerdict i8_exact_tile(int blocks) {
    uint64_t rng = 0x3F84D5B5B5470917ull;
    std::vector<int8_t> A(1024), B(1024);
    std::vector<int32_t> C(256), ref(256);
    for (int8_t& v : A) v = (int8_t)(lcg_bits(rng) & 0xff);
    for (int8_t& v : B) v = (int8_t)(lcg_bits(rng) & 0xff);
    for (int32_t& v : C) v = (int32_t)(lcg_bits(rng) & 0x7fffffff) - (1 << 30);
    for (int i = 0; i < 16; i++)
        for (int j = 0; j < 16; j++) {
            int64_t s = C[i * 16 + j];
            for (int k = 0; k < 64; k++) s += (int)A[i * 64 + k] * (int)B[k * 16 + j];
            ref[i * 16 + j] = (int32_t)s;
        }
    return judge_tile(run_i8_tile(A.data(), B.data(), C.data(), blocks), ref);
}

// Sparse exact tile: integer-valued f16 in -16..16 (never 0 in A, so every
// kept slot counts); group g of row i keeps the ascending position pair
// number (i + g) % 6 of (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), so all six occur
// in every row and every group column. 32 products of at most 256: integers
// below 2^24 under any order.
TileVerdict sparse_exact_tile(int blocks) {
    static const uint8_t PAIRS[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
    uint64_t rng = 0x9216D5D98979FB1Bull;
    std::vector<int> a(512), b(1024);
    std::vector<uint16_t> A(512), B(1024);
    std::vector<uint8_t> idx(512);
    for (int i = 0; i < 512; i++) {
        int v = lcg_int(rng, 15);
        A[i] = f16_bits_of_int(a[i] = v >= 0 ? v + 1 : v);
    }
    for (int i = 0; i < 1024; i++) B[i] = f16_bits_of_int(b[i] = lcg_int(rng, 16));
    for (int i = 0; i < 16; i++)
        for (int e = 0; e < 32; e++) idx[i * 32 + e] = PAIRS[(i + (e >> 1)) % 6][e & 1];
    std::vector<float> ref(256);
    for (int i = 0; i < 16; i++)
        for (int j = 0; j < 16; j++) {
            int s = 0;
            for (int e = 0; e < 32; e++)
                s += a[i * 32 + e] * b[(4 * (e >> 1) + idx[i * 32 + e]) * 16 + j];
            ref[i * 16 + j] = (float)s;
        }
    return judge_tile(run_smfmac_tile(A.data(), idx.data(), B.data(), blocks), ref);
}

// FP64 / FP16 / INT8 / 2:4-sparse matrix-core probe: one fixed exact tile per
// form on 2 blocks per CU (slab 0 bitwise against the host product, every
// other slab bitwise against slab 0), then a timed f64 and i8 burn, each after
// a warm-up launch, whose waves must all agree bit for bit.
py::dict mfma_probe_formats(int dev, int burn_iters) {
    require_dev(dev);
    require(burn_iters > 0, "burn_iters must be > 0");
    HIP_CHECK(hipSetDevice(dev));
    int blocks = std::min(compute_units(dev) * 2, MAX_TILE_BLOCKS);
    TileVerdict f64 = f64_exact_tile(blocks);
    TileVerdict f16 = f16_exact_tile(blocks);
    TileVerdict i8 = i8_exact_tile(blocks);
    TileVerdict sp = sparse_exact_tile(blocks);
    int burn_grid = burn_blocks(dev, 0, 2);   // 2 × 256-thread WGs per CU
    // operations per block and iteration: 4 waves/WG × accumulators × 2·M·N·K
    TimedBurn b64 = timed_burn(launch_f64_burn, burn_grid, burn_iters,
                               4.0 * FMT_BURN_ACCS * 2.0 * 16 * 16 * 4);
    TimedBurn b8 = timed_burn(launch_i8_burn, burn_grid, burn_iters,
                              4.0 * FMT_BURN_ACCS * 2.0 * 16 * 16 * 64);
    py::dict d;
    d["f64_ok"] = f64.ok;
    d["f16_ok"] = f16.ok;
    d["i8_ok"] = i8.ok;
    d["sparse_f16_ok"] = sp.ok;
    d["f64_slab_mismatches"] = f64.bad_slabs;
    d["f16_slab_mismatches"] = f16.bad_slabs;
    d["i8_slab_mismatches"] = i8.bad_slabs;
    d["sparse_f16_slab_mismatches"] = sp.bad_slabs;
    d["f64_tflops"] = b64.tflops;
    d["i8_tops"] = b8.tflops;
    d["f64_burn_mismatches"] = b64.mismatches;
    d["i8_burn_mismatches"] = b8.mismatches;
    d["f64_burn_ms"] = b64.ms;
    d["i8_burn_ms"] = b8.ms;
    d["blocks"] = blocks;
    return d;
}

}  // namespace

PYBIND11_MODULE(_gpuprobe_formats, m) {
    m.doc() = "MI355X (gfx950) FP64 / FP16 / INT8 / 2:4-sparse matrix-core probes";
    m.def("mfma_f64_tile_run", &mfma_f64_tile_run, py::arg("dev"), py::arg("A"),
          py::arg("B"), py::arg("C") = py::none(), py::arg("blocks") = 1);
    m.def("mfma_f16_tile_run", &mfma_f16_tile_run, py::arg("dev"), py::arg("A_bits"),
          py::arg("B_bits"), py::arg("blocks") = 1);
    m.def("mfma_i8_tile_run", &mfma_i8_tile_run, py::arg("dev"), py::arg("A"),
          py::arg("B"), py::arg("C") = py::none(), py::arg("blocks") = 1);
    m.def("smfmac_f16_tile_run", &smfmac_f16_tile_run, py::arg("dev"), py::arg("A_bits"),
          py::arg("A_idx"), py::arg("B_bits"), py::arg("blocks") = 1);
    m.def("mfma_f64_burn_run", &mfma_f64_burn_run, py::arg("dev") = 0,
          py::arg("iters") = 64, py::arg("blocks") = 0);
    m.def("mfma_i8_burn_run", &mfma_i8_burn_run, py::arg("dev") = 0,
          py::arg("iters") = 64, py::arg("blocks") = 0);
    m.def("mfma_probe_formats", &mfma_probe_formats, py::arg("dev") = 0,
          py::arg("burn_iters") = 20000);
}
