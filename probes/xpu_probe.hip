// kata_xpu_device_plugin_amd._gpuprobe — MI355X (gfx950) health/burn-in probes.
//
// A device plugin hands whole GPUs to Kata VMs; before a GPU is advertised
// (or after a RAS event) the operator wants evidence the silicon is sane.
// The reference has no such capability (NVML-less); these
// CDNA4-native probes are the MI355X answer:
//
//   * hbm_bandwidth_probe : float4-coalesced streaming copy (16 B/lane per
//     instruction — cdna_hip_programming.md §2 coalescing rule), grid ≫256
//     workgroups to fill all 8 XCDs; a healthy MI355X sustains ≈6.3 TB/s
//     (MI355X_MICROARCH.md: 8 TB/s peak, 79% achievable).
//     One pattern-checked copy after timing reports copy_mismatches.
//   * mfma_probe_f32  : v_mfma_f32_16x16x4_f32 tile with the documented
//     lane mapping (A[l&15][l>>4], B[l>>4][l&15]; C/D col=l&15,
//     row=(l>>4)*4+reg — cdna_hip_programming.md §3) on full-mantissa
//     inputs, 2 blocks per CU. Slab 0 must equal the host's k-ordered fmaf
//     chain bit for bit (measured on MI355X: it does, subnormal products,
//     inputs and C included) and every other slab must equal slab 0.
//   * mfma_probe_bf16 : v_mfma_f32_32x32x16_bf16 tile on 2 blocks per CU,
//     within 16·2^-23·Σ|a·b| of an fp64 reference (the hardware's summation
//     order is not documented, so no bitwise claim) and bit-identical across
//     blocks; then a throughput burn (the CDNA4 matrix-core rate, ~2.5 PF
//     dense chip-wide) whose waves must all agree bit for bit.
//   * mfma_probe_lowp : the low-precision matrix-core paths tenants buy the
//     part for. v_mfma_f32_16x16x32_fp8_fp8 and the CDNA4-only
//     v_mfma_scale_f32_16x16x128_f8f6f4 (OCP e4m3 and e2m1 operands, E8M0
//     block scales) each run a fixed tile whose fp64 product is exact in f32
//     under any summation order, on 2 blocks per CU: slab 0 bitwise against
//     the host, every slab bitwise against slab 0. Then an MX-fp8 and an
//     MX-fp4 throughput burn (~5 PF and ~10 PF dense chip-wide) whose waves
//     must all agree bit for bit. FP6 is not probed (FP4's datapath and rate).
//   * lds_bandwidth_probe : ds_read_b128 streaming; the warm-up launch's
//     sums are checked exactly, so the reads hit the slots the rate assumes.
//   * hbm_latency_probe : pointer chase; the final index must equal the
//     host's walk of the same chain.
//   * memtest         : address-pattern write/readback over a buffer,
//     returns mismatch count (catches dead HBM channels). corrupt_offsets
//     flips words of the live buffer between write and check, to show the
//     probe can fail.
//   * unit_sweep      : one LDS-exclusive workgroup per CU puts the exact tiles
//     above through every SIMD, checks the CU's whole LDS allocation, and
//     records the hardware ids (XCD / SE / CU / SIMD) each wave ran on, so
//     coverage is shown and a failure has an address. poison is its test hook.
//   * *_run / hbm_copy_check : raw entry points that return what a kernel
//     computed, for tests against independent references.
//
// The matrix-core lane maps are stated once, in mfma_forms.h; the tile kernels
// and the unit sweep both run on those forms.
//
// Wavefront size is 64 everywhere (gfx950; cdna_hip_programming.md §1).
// Build: hipcc --offload-arch=gfx950 (driven by setup.py / __graft_entry__).

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
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

namespace py = pybind11;

namespace {

// ---------------------------------------------------------------------------
// HBM bandwidth: grid-stride float4 copy. 256 threads/WG, ≥2048 WGs so all
// 8 XCDs × 32 CUs are saturated (a launch needs ≫256 workgroups to fill
// the chip — MI355X_MICROARCH.md §Workgroup dispatch).
// ---------------------------------------------------------------------------
__global__ void copy_f4(const float4* __restrict__ src,
                        float4* __restrict__ dst, size_t n4) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n4; i += stride) dst[i] = src[i];
}

// ---------------------------------------------------------------------------
// Address-pattern memtest: write f(i), read back, count mismatches on GPU.
// ---------------------------------------------------------------------------
__global__ void pattern_write(uint64_t* __restrict__ buf, size_t n, uint64_t salt) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) buf[i] = (uint64_t)i * 0x9E3779B97F4A7C15ull ^ salt;
}

__global__ void pattern_check(const uint64_t* __restrict__ buf, size_t n,
                              uint64_t salt, unsigned long long* mismatches) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t stride = (size_t)gridDim.x * blockDim.x;
    unsigned long long local = 0;
    for (; i < n; i += stride)
        if (buf[i] != ((uint64_t)i * 0x9E3779B97F4A7C15ull ^ salt)) local++;
    if (local) atomicAdd(mismatches, local);
}

// ---------------------------------------------------------------------------
// LDS bandwidth burn: ds_read_b128 streaming from a 32 KiB per-WG tile.
// Per the §LDS table (MI355X_MICROARCH.md) b128 reads move 256 B/clk/CU
// (≈150 TB/s chip-wide from ≥4 waves/CU); one scalar accumulate per read
// keeps the loop LDS-bound (4 LDS cycles vs 2 VALU cycles per b128).
// A sick CU/LDS array shows up as a chip-wide rate far below spec.
// ---------------------------------------------------------------------------
typedef float lds_f32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(256, 4)
lds_read_burn(float* __restrict__ out, int iters) {
    __shared__ lds_f32x4 buf[2048];  // 32 KiB → 4 WGs/CU fit in 160 KiB
    for (int i = threadIdx.x; i < 2048; i += 256) {
        lds_f32x4 v = {(float)i, 1.f, 2.f, 3.f};
        buf[i] = v;
    }
    __syncthreads();
    // Inline-asm ds_read_b128 (volatile): plain C++ float4 reads get their
    // unused components dead-code-eliminated into ds_read_b32, which
    // measures the 128 B/clk narrow-read rate instead of the 256 B/clk
    // b128 rate (§LDS table). One scalar accumulate per read keeps the
    // loop LDS-bound (8×4 LDS cycles vs 8×2 VALU per batch); the explicit
    // s_waitcnt is mandatory — hipcc pads nothing inside asm (§5.7).
    // The address comes from buf itself and the asm clobbers "memory": with a
    // bare byte offset and no clobber the compiler sees buf written and never
    // read, deletes the fill and allocates no LDS at all, and every read
    // returns 0 from outside the (empty) allocation. Outputs are
    // early-clobber: the address register is read by all eight instructions.
    typedef __attribute__((address_space(3))) lds_f32x4 lds_slot;
    unsigned base = (unsigned)(size_t)(lds_slot*)&buf[threadIdx.x & 255];  // lane-contiguous 16-B slots
    float acc = 0.f;
    for (int it = 0; it < iters; it++) {
        lds_f32x4 v0, v1, v2, v3, v4, v5, v6, v7;
        asm volatile(
            "ds_read_b128 %0, %8 offset:0\n\t"
            "ds_read_b128 %1, %8 offset:4096\n\t"
            "ds_read_b128 %2, %8 offset:8192\n\t"
            "ds_read_b128 %3, %8 offset:12288\n\t"
            "ds_read_b128 %4, %8 offset:16384\n\t"
            "ds_read_b128 %5, %8 offset:20480\n\t"
            "ds_read_b128 %6, %8 offset:24576\n\t"
            "ds_read_b128 %7, %8 offset:28672\n\t"
            "s_waitcnt lgkmcnt(0)"
            : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3),
              "=&v"(v4), "=&v"(v5), "=&v"(v6), "=&v"(v7)
            : "v"(base)
            : "memory");
        acc += v0.x + v1.x + v2.x + v3.x + v4.x + v5.x + v6.x + v7.x;
    }
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = acc;
}

// ---------------------------------------------------------------------------
// HBM load-to-use latency: single-wave pointer chase over a permutation
// too large for L2/LLC (guide: ~900 cycles per HBM-miss dependent load).
// ---------------------------------------------------------------------------
__global__ void pointer_chase(const uint32_t* __restrict__ next,
                              uint32_t* __restrict__ out, int steps) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t idx = 0;
    for (int i = 0; i < steps; i++) idx = next[idx];
    *out = idx;  // keep the chain live
}

// ---------------------------------------------------------------------------
// Matrix-core tile kernels: one wave per block, every block the same tile into
// its own slab (form_tile). The lane maps are in mfma_forms.h.
// ---------------------------------------------------------------------------
__global__ void mfma_f32_tile(const float* __restrict__ A,  // 16×4 row-major
                              const float* __restrict__ B,  // 4×16 row-major
                              const float* __restrict__ C,  // 16×16 or nullptr (= 0)
                              float* __restrict__ D) {      // gridDim.x × 16×16
    form_tile<MfmaF32x16x16x4>({A, B}, C, D);
}

__global__ void mfma_bf16_tile(const __bf16* __restrict__ A,  // 32×16 row-major
                               const __bf16* __restrict__ B,  // 16×32 row-major
                               float* __restrict__ D) {       // gridDim.x × 32×32
    form_tile<Mfma32x32x16<__bf16>>({A, B}, nullptr, D);
}

template <int AF, int BF>
__global__ void mfma_fp8_tile(const uint8_t* __restrict__ A,  // 16×32 codes
                              const uint8_t* __restrict__ B,  // 32×16 codes
                              float* __restrict__ D) {        // gridDim.x × 16×16
    form_tile<MfmaFp8x16x16x32<AF, BF>>({A, B}, nullptr, D);
}

template <int AF, int BF>
__global__ void mfma_mx_tile(const uint8_t* __restrict__ A,   // 16×128 codes
                             const uint8_t* __restrict__ B,   // 128×16 codes
                             const uint8_t* __restrict__ SA,  // 16×4 E8M0
                             const uint8_t* __restrict__ SB,  // 4×16 E8M0
                             float* __restrict__ D) {         // gridDim.x × 16×16
    form_tile<MfmaMx16x16x128<AF, BF>>({A, B, SA, SB}, nullptr, D);
}

// Throughput burn: every wave hammers independent accumulators with
// back-to-back 32×32×16 bf16 MFMAs (32 cyc/SIMD issue; 4 accumulators give
// plenty of independence). Result is summed into out so the work is live.
__global__ void __launch_bounds__(256, 2)
mfma_bf16_burn(float* __restrict__ out, int iters) {
    int l = threadIdx.x & (WAVE - 1);
    bf16x8 a, b;
    for (int j = 0; j < 8; j++) {
        a[j] = (__bf16)(0.5f + 0.001f * (float)((l + j) & 7));
        b[j] = (__bf16)(0.25f + 0.002f * (float)((l ^ j) & 7));
    }
    f32x16 acc0 = {}, acc1 = {}, acc2 = {}, acc3 = {};
    for (int it = 0; it < iters; it++) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc3, 0, 0, 0);
    }
    float s = 0;
    for (int r = 0; r < 16; r++) s += acc0[r] + acc1[r] + acc2[r] + acc3[r];
    // one store per lane; never zero, so the compiler cannot DCE the loop
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// Throughput burn on the instruction the tile tests verified. Element e of
// lane l (k = mx_k(l>>4, e) of row or column l&15) is the code of the integer
// 1 + (l+e)%3 for A and 1 + (l^e)%3 for B, so the operand map matters; both
// scales are 127 (×1). Accumulator n starts at n, which keeps the eight
// chains distinct for the compiler, and every partial sum is an exact
// integer: one MFMA adds at most 128·9 = 1152 to an element, so the per-lane
// sum, at most 112 + 32·1152·iters, stays below 2^24 for iters ≤ 455 (and a
// single accumulator up to iters = 14563). Longer burns round, identically in
// every wave.
// Eight independent accumulators per wave and two waves per SIMD: the
// dependent-accumulator latency of this form is not documented, and eight
// back-to-back issues (8×16 cycles at the FP4 rate) cover any plausible one.
// Measured on MI355X: ≈4300 TF MX-fp8, ≈8200 TF MX-fp4 (profiles/mfma_lowp.md).
constexpr int MX_BURN_ACCS = 8;

template <int FMT>
__global__ void __launch_bounds__(256, 2)
mfma_mx_burn(float* __restrict__ out, int iters) {
    int l = threadIdx.x & (WAVE - 1);
    // codes of 1, 2, 3
    constexpr uint32_t c1 = FMT == FMT_E2M1 ? 0x2 : 0x38;
    constexpr uint32_t c2 = FMT == FMT_E2M1 ? 0x4 : 0x40;
    constexpr uint32_t c3 = FMT == FMT_E2M1 ? 0x5 : 0x44;
    uint8_t ca[32], cb[32];
#pragma unroll
    for (int e = 0; e < 32; e++) {
        int va = (l + e) % 3, vb = (l ^ e) % 3;
        ca[e] = (uint8_t)(va == 0 ? c1 : va == 1 ? c2 : c3);
        cb[e] = (uint8_t)(vb == 0 ? c1 : vb == 1 ? c2 : c3);
    }
    i32x8 a = pack_mx<FMT>(ca), b = pack_mx<FMT>(cb);
    f32x4 acc[MX_BURN_ACCS];
#pragma unroll
    for (int n = 0; n < MX_BURN_ACCS; n++) acc[n] = {(float)n, (float)n, (float)n, (float)n};
    for (int it = 0; it < iters; it++) {
#pragma unroll
        for (int n = 0; n < MX_BURN_ACCS; n++)
            acc[n] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
                a, b, acc[n], FMT, FMT, 0, 127, 0, 127);
    }
    float s = 0;
#pragma unroll
    for (int n = 0; n < MX_BURN_ACCS; n++) s += acc[n][0] + acc[n][1] + acc[n][2] + acc[n][3];
    // one store per lane
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

// ---------------------------------------------------------------------------
// Unit sweep: the probes' exact tiles through every SIMD of every CU, with a
// record of where each wave ran.
//
// One workgroup asks for more than half of a CU's 160 KiB of LDS, so two can
// never share a CU; a grid of one workgroup per CU whose workgroups outlive
// the dispatcher's start spread (0.34–0.69 µs for 1024 blocks) therefore has
// one on every CU at once. Nothing else is assumed about placement: each wave
// reads HW_REG_HW_ID (wave slot, SIMD, CU, SH, SE) and HW_REG_XCC_ID (XCD)
// and the host decides from the records which units were covered. A workgroup
// never waits for another one.
//
// Every wave recomputes each selected tile `reps` times from a zero
// accumulator and compares its registers bit for bit with the golden tile the
// host supplies, through the forms of mfma_forms.h: the inputs, lane maps and
// instructions of the tile kernels above. The inputs are loop-invariant and
// the MFMA builtins are pure, so one operand goes through an empty volatile
// asm in each repetition: without it the compiler computes the tile once,
// outside the loop.
//
// LDS: the workgroup fills its whole allocation with an address pattern and
// reads it back mirrored (word i was written by thread i % n and is read by
// thread n-1 - i % n, which sits in another wave), counting wrong words.
//
// Poison is the test hook that shows the sweep can fail: a wave whose own
// hardware ids match XORs poison_xor into element 0 of lane 0 of that kind's
// result in every repetition, or (kind = lds) into one word of the
// workgroup's own allocation between fill and read-back.
//
// Record per wave, eight uint32: hw_id, xcc_id, then the wrong-element counts
// of f32, bf16, fp8, mx_fp8, mx_fp4 and the wave's share of wrong LDS words.
// ---------------------------------------------------------------------------
enum SweepKind { SK_F32 = 0, SK_BF16, SK_FP8, SK_MX_FP8, SK_MX_FP4, SK_LDS, SK_COUNT };

constexpr int SWEEP_RECORD_WORDS = 8;
constexpr size_t CU_LDS_BYTES = 160 << 10;

struct SweepInputs {
    float a32[64], b32[64], g32[256];
    uint16_t a16[512], b16[512];
    float g16[1024];
    uint8_t a8[512], b8[512];
    float g8[256];
    uint8_t amx8[2048], bmx8[2048], samx8[64], sbmx8[64];
    float gmx8[256];
    uint8_t amx4[2048], bmx4[2048], samx4[64], sbmx4[64];
    float gmx4[256];
};

struct SweepParams {
    uint32_t kinds;      // bit k set = SweepKind k selected
    int reps;
    uint32_t lds_words;  // the dynamic LDS allocation; a multiple of blockDim.x
    int poison_kind;     // a SweepKind, or -1
    uint32_t poison_xcc, poison_cu_key, poison_simd, poison_xor;
};

// s_getreg_b32 immediate: register id, bit offset 0, all 32 bits.
constexpr int sweep_hwreg(int id) { return id | (31 << 11); }
constexpr int HWREG_HW_ID = 4, HWREG_XCC_ID = 20;

// Makes `v` opaque to the compiler at this point of every repetition.
template <class V>
__device__ __forceinline__ void sweep_relive(V& v) {
    static_assert(sizeof(V) % 4 == 0, "whole registers");
    uint32_t w[sizeof(V) / 4];
    __builtin_memcpy(w, &v, sizeof(V));
    asm volatile("" : "+v"(w[0]));
    __builtin_memcpy(&v, w, sizeof(V));
}

template <int N, class Acc>
__device__ __forceinline__ uint32_t sweep_count_bad(const Acc& acc, const float (&gold)[N],
                                                    uint32_t flip) {
    uint32_t bad = 0;
#pragma unroll
    for (int j = 0; j < N; j++) {
        uint32_t got = __float_as_uint(acc[j]);
        if (j == 0) got ^= flip;
        bad += got != __float_as_uint(gold[j]);
    }
    return bad;
}

__device__ __forceinline__ uint32_t sweep_wave_sum(uint32_t v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// One form's tile, `reps` times on this wave: the lane's wrong-element count.
template <class Form>
__device__ __forceinline__ uint32_t sweep_form(const typename Form::In& in,
                                               const float* __restrict__ G, int l, int reps,
                                               uint32_t flip) {
    typename Form::Frag f = Form::load(in, l);
    float gold[Form::REGS];
#pragma unroll
    for (int reg = 0; reg < Form::REGS; reg++) gold[reg] = G[Form::d_index(l, reg)];
    uint32_t n = 0;
    for (int r = 0; r < reps; r++) {
        sweep_relive(f.a);
        typename Form::Acc acc = {};
        acc = Form::mma(f, acc);
        n += sweep_count_bad<Form::REGS>(acc, gold, flip);
    }
    return n;
}

__global__ void __launch_bounds__(1024)
unit_sweep(const SweepInputs* __restrict__ in, SweepParams p, uint32_t* __restrict__ records) {
    extern __shared__ uint32_t sweep_lds[];
    const int l = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint32_t hw_id = __builtin_amdgcn_s_getreg(sweep_hwreg(HWREG_HW_ID));
    const uint32_t xcc_id = __builtin_amdgcn_s_getreg(sweep_hwreg(HWREG_XCC_ID));
    const bool on_cu = p.poison_kind >= 0 && (xcc_id & 15u) == p.poison_xcc &&
                       ((hw_id >> 8) & 255u) == p.poison_cu_key;
    const bool on_simd = on_cu && ((hw_id >> 4) & 3u) == p.poison_simd;
    auto flip_for = [&](int kind) -> uint32_t {
        return on_simd && p.poison_kind == kind && l == 0 ? p.poison_xor : 0u;
    };
    uint32_t bad[SK_COUNT] = {0, 0, 0, 0, 0, 0};

    if (p.kinds & (1u << SK_LDS)) {
        const uint32_t n = blockDim.x, words = p.lds_words;
        for (uint32_t i = threadIdx.x; i < words; i += n)
            sweep_lds[i] = i * 0x9E3779B9u ^ 0xA5A55A5Au;
        __syncthreads();
        // words >= n >= 64, so the flipped word lies inside the allocation
        if (on_cu && p.poison_kind == SK_LDS && threadIdx.x == 0)
            sweep_lds[words / 2 + 1] ^= p.poison_xor;
        __syncthreads();
        uint32_t wrong = 0;
        for (uint32_t i = threadIdx.x; i < words; i += n) {
            uint32_t j = words - 1 - i;
            wrong += sweep_lds[j] != (j * 0x9E3779B9u ^ 0xA5A55A5Au);
        }
        bad[SK_LDS] = sweep_wave_sum(wrong);
    }

    if (p.kinds & (1u << SK_F32))
        bad[SK_F32] = sweep_wave_sum(sweep_form<MfmaF32x16x16x4>(
            {in->a32, in->b32}, in->g32, l, p.reps, flip_for(SK_F32)));
    if (p.kinds & (1u << SK_BF16))
        bad[SK_BF16] = sweep_wave_sum(sweep_form<Mfma32x32x16<__bf16>>(
            {reinterpret_cast<const __bf16*>(in->a16), reinterpret_cast<const __bf16*>(in->b16)},
            in->g16, l, p.reps, flip_for(SK_BF16)));
    if (p.kinds & (1u << SK_FP8))
        bad[SK_FP8] = sweep_wave_sum(sweep_form<MfmaFp8x16x16x32<FMT_E4M3, FMT_E4M3>>(
            {in->a8, in->b8}, in->g8, l, p.reps, flip_for(SK_FP8)));
    if (p.kinds & (1u << SK_MX_FP8))
        bad[SK_MX_FP8] = sweep_wave_sum(sweep_form<MfmaMx16x16x128<FMT_E4M3, FMT_E4M3>>(
            {in->amx8, in->bmx8, in->samx8, in->sbmx8}, in->gmx8, l, p.reps,
            flip_for(SK_MX_FP8)));
    if (p.kinds & (1u << SK_MX_FP4))
        bad[SK_MX_FP4] = sweep_wave_sum(sweep_form<MfmaMx16x16x128<FMT_E2M1, FMT_E2M1>>(
            {in->amx4, in->bmx4, in->samx4, in->sbmx4}, in->gmx4, l, p.reps,
            flip_for(SK_MX_FP4)));

    if (l == 0) {
        uint32_t* rec = records +
            ((size_t)blockIdx.x * (blockDim.x / WAVE) + wave) * SWEEP_RECORD_WORDS;
        rec[0] = hw_id;
        rec[1] = xcc_id;
        rec[2] = bad[SK_F32];
        rec[3] = bad[SK_BF16];
        rec[4] = bad[SK_FP8];
        rec[5] = bad[SK_MX_FP8];
        rec[6] = bad[SK_MX_FP4];
        rec[7] = bad[SK_LDS];
    }
}

// ---------------------------------------------------------------------------
// Host-side wrappers. The argument checks (run before the first HIP call of
// every entry point), the RAII handles and the launch, fetch, timing and
// comparison helpers are in probe_host.h, shared with xpu_probe_formats.hip.
// ---------------------------------------------------------------------------

// "e4m3" / "e5m2" / "e2m1" → the instruction's format number, if the entry
// point allows that format.
int parse_fmt(const std::string& s, std::initializer_list<int> allowed, const char* what) {
    int f = s == "e4m3" ? FMT_E4M3 : s == "e5m2" ? FMT_E5M2 : s == "e2m1" ? FMT_E2M1 : -1;
    require(std::find(allowed.begin(), allowed.end(), f) != allowed.end(), what);
    return f;
}

int device_count() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) return 0;
    return n;
}

py::dict device_info(int dev) {
    require_dev(dev);
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    size_t free_b = 0, total_b = 0;
    HIP_CHECK(hipSetDevice(dev));
    HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
    py::dict d;
    d["name"] = std::string(prop.name);
    d["gcn_arch"] = std::string(prop.gcnArchName);
    d["compute_units"] = prop.multiProcessorCount;
    d["total_mem_bytes"] = (uint64_t)total_b;
    d["free_mem_bytes"] = (uint64_t)free_b;
    d["pci_bus_id"] = prop.pciBusID;
    d["pci_domain_id"] = prop.pciDomainID;
    d["pci_device_id"] = prop.pciDeviceID;
    d["warp_size"] = prop.warpSize;
    return d;
}

constexpr uint64_t PATTERN_SALT = 0xA5A5A5A55A5A5A5Aull;

// Fill the `n` 64-bit words at `w` with the memtest address pattern, run
// `between`, and count the words at `r` that do not hold the pattern.
template <class F>
uint64_t pattern_mismatches(uint64_t* w, const uint64_t* r, size_t n, int blocks,
                            F&& between) {
    DevBuf mm(sizeof(unsigned long long));
    HIP_CHECK(hipMemset(mm.p, 0, sizeof(unsigned long long)));
    hipLaunchKernelGGL(pattern_write, dim3(blocks), dim3(256), 0, 0, w, n, PATTERN_SALT);
    HIP_CHECK(hipGetLastError());
    between();
    hipLaunchKernelGGL(pattern_check, dim3(blocks), dim3(256), 0, 0, r, n, PATTERN_SALT,
                       mm.as<unsigned long long>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    unsigned long long mismatches = 0;
    HIP_CHECK(hipMemcpy(&mismatches, mm.p, sizeof(mismatches), hipMemcpyDeviceToHost));
    return mismatches;
}

void launch_copy(int blocks, const float4* src, float4* dst, size_t n4) {
    hipLaunchKernelGGL(copy_f4, dim3(blocks), dim3(256), 0, 0, src, dst, n4);
}

// Pattern-checked copy: fill src with the memtest address pattern, clear dst,
// run copy_f4 and count the 64-bit words of dst that do not hold the pattern.
// The pattern differs at every word, so a copy from the wrong index, a
// skipped element or a short loop bound all show up in the count.
uint64_t checked_copy(float4* src, float4* dst, size_t n4, int blocks) {
    HIP_CHECK(hipMemset(dst, 0, n4 * sizeof(float4)));
    return pattern_mismatches((uint64_t*)src, (const uint64_t*)dst, n4 * 2, blocks, [&] {
        launch_copy(blocks, src, dst, n4);
        HIP_CHECK(hipGetLastError());
    });
}

py::dict hbm_copy_check(int dev, size_t bytes) {
    require_dev(dev);
    require(bytes >= sizeof(float4), "bytes must hold at least one float4 (16)");
    HIP_CHECK(hipSetDevice(dev));
    size_t n4 = bytes / sizeof(float4);
    int blocks = compute_units(dev) * 8;
    DevBuf src(n4 * sizeof(float4)), dst(n4 * sizeof(float4));
    py::dict d;
    d["mismatches"] = checked_copy(src.as<float4>(), dst.as<float4>(), n4, blocks);
    d["bytes"] = (uint64_t)(n4 * sizeof(float4));
    return d;
}

py::dict hbm_bandwidth_probe(int dev, size_t bytes, int iters) {
    require_dev(dev);
    require(bytes >= sizeof(float4), "bytes must hold at least one float4 (16)");
    require(iters > 0, "iters must be > 0");
    HIP_CHECK(hipSetDevice(dev));
    size_t n4 = bytes / sizeof(float4);
    DevBuf src_buf(n4 * sizeof(float4)), dst_buf(n4 * sizeof(float4));
    float4 *src = src_buf.as<float4>(), *dst = dst_buf.as<float4>();
    HIP_CHECK(hipMemset(src, 0x3c, n4 * sizeof(float4)));
    int blocks = compute_units(dev) * 8;  // ≫256 WGs, fills all XCDs
    auto copy = [&] { launch_copy(blocks, src, dst, n4); };
    copy();  // warmup
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float best_ms = best_timed_ms(iters, copy);
    // one pattern-checked copy after timing: the rate above says nothing
    // about whether dst ever equalled src
    uint64_t copy_mismatches = checked_copy(src, dst, n4, blocks);
    double gbps = 2.0 * (double)(n4 * sizeof(float4)) / (best_ms * 1e6);
    py::dict d;
    d["gbps"] = gbps;
    d["best_ms"] = best_ms;
    d["bytes_moved"] = (uint64_t)(2 * n4 * sizeof(float4));
    d["copy_mismatches"] = copy_mismatches;
    return d;
}

// lds_read_burn lane t reads slots t, t+256, …, t+1792, whose .x hold their
// own index, so one iteration adds 8t + 256·(0+…+7) = 8t + 7168. All partial
// sums are integers; they stay exact in f32 while iters·9208 < 2^24.
constexpr int LDS_EXACT_ITERS = 1822;

uint64_t lds_mismatches(const std::vector<float>& out, int iters) {
    uint64_t bad = 0;
    for (size_t i = 0; i < out.size(); i++)
        if (out[i] != (float)iters * (float)(8 * (int)(i & 255) + 7168)) bad++;
    return bad;
}

void launch_lds_burn(int blocks, float* out, int iters) {
    hipLaunchKernelGGL(lds_read_burn, dim3(blocks), dim3(256), 0, 0, out, iters);
}

py::bytes lds_read_burn_run(int dev, int iters, int blocks) {
    require_dev(dev);
    require(iters > 0, "iters must be > 0");
    require_burn_blocks(blocks);
    HIP_CHECK(hipSetDevice(dev));
    blocks = burn_blocks(dev, blocks, 4);
    return as_bytes(launch_fetch((size_t)blocks * 256, [&](float* out) {
        launch_lds_burn(blocks, out, iters);
    }));
}

py::dict lds_bandwidth_probe(int dev, int iters) {
    require_dev(dev);
    require(iters > 0, "iters must be > 0");
    HIP_CHECK(hipSetDevice(dev));
    int blocks = burn_blocks(dev, 0, 4);   // 4 × 32 KiB per CU
    std::vector<float> warm((size_t)blocks * 256);
    DevBuf out_buf(warm.size() * 4);
    float* out = out_buf.as<float>();
    static_assert(256 <= LDS_EXACT_ITERS, "warm-up sums must stay exact");
    launch_lds_burn(blocks, out, 256);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    // the warm-up launch doubles as the read-address check (exact sums); the
    // timed launch reuses its buffer, so nothing is allocated in between
    HIP_CHECK(hipMemcpy(warm.data(), out, warm.size() * 4, hipMemcpyDeviceToHost));
    uint64_t mismatches = lds_mismatches(warm, 256);
    float ms = timed_ms([&] { launch_lds_burn(blocks, out, iters); });
    // bytes: blocks × 256 lanes × 8 b128-reads × 16 B per iteration
    double bytes = (double)blocks * 256 * 8 * 16 * (double)iters;
    py::dict d;
    d["tbps"] = bytes / (ms * 1e9);
    d["burn_ms"] = ms;
    d["mismatches"] = mismatches;
    return d;
}

py::dict hbm_latency_probe(int dev, size_t bytes, int steps) {
    require_dev(dev);
    require(steps > 0, "steps must be > 0");
    // n >= 2 for the Sattolo loop below; indices are uint32_t
    require(bytes >= 8, "bytes must hold at least two uint32 (8)");
    require(bytes / 4 <= ((size_t)1 << 32), "bytes / 4 must not exceed 2^32");
    HIP_CHECK(hipSetDevice(dev));
    size_t n = bytes / sizeof(uint32_t);
    // Sattolo shuffle → one full cycle; stride-randomized to defeat
    // prefetch and the 256 MiB LLC (use ≥1 GiB).
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; i++) perm[i] = (uint32_t)i;
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    for (size_t i = n - 1; i > 0; i--) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        size_t j = (size_t)(rng % i);
        std::swap(perm[i], perm[j]);
    }
    std::vector<uint32_t> next(n);
    for (size_t i = 0; i < n; i++) next[perm[i]] = perm[(i + 1) % n];
    // the host holds the chain: where `steps` hops from 0 must end
    uint32_t expected = 0;
    for (int i = 0; i < steps; i++) expected = next[expected];
    DevBuf next_buf = upload(next.data(), n * 4), out_buf(4);
    uint32_t *d_next = next_buf.as<uint32_t>(), *d_out = out_buf.as<uint32_t>();
    auto chase = [&](int hops) {
        hipLaunchKernelGGL(pointer_chase, dim3(1), dim3(64), 0, 0, d_next, d_out, hops);
    };
    chase(1000);  // warmup
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float ms = timed_ms([&] { chase(steps); });
    uint32_t final_index = 0;
    HIP_CHECK(hipMemcpy(&final_index, d_out, 4, hipMemcpyDeviceToHost));
    py::dict d;
    d["latency_ns"] = ms * 1e6 / steps;
    d["steps"] = steps;
    d["final_index"] = final_index;
    d["expected_index"] = expected;
    return d;
}

py::dict pcie_bandwidth_probe(int dev, size_t bytes, int iters) {
    require_dev(dev);
    require(bytes >= 1, "bytes must be >= 1");
    require(iters > 0, "iters must be > 0");
    // Host-link health: pinned-memory H2D/D2H streaming. MI355X host link
    // is PCIe Gen5 x16 (63 GB/s spec); a degraded link (wrong slot width,
    // retraining) shows up far below that.
    HIP_CHECK(hipSetDevice(dev));
    HostBuf host(bytes);
    DevBuf d(bytes);
    std::memset(host.p, 0x5a, bytes);
    auto run = [&](bool h2d) {
        auto copy = [&] {
            HIP_CHECK(hipMemcpyAsync(h2d ? d.p : host.p, h2d ? host.p : d.p, bytes,
                                     h2d ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, 0));
        };
        copy();  // warmup
        HIP_CHECK(hipDeviceSynchronize());
        return (double)bytes / (best_timed_ms(iters, copy) * 1e6);
    };
    double h2d = run(true);
    double d2h = run(false);
    py::dict r;
    r["h2d_gbps"] = h2d;
    r["d2h_gbps"] = d2h;
    r["bytes"] = (uint64_t)bytes;
    return r;
}

// corrupt_offsets is a test hook that shows the probe can fail: between the
// write and the check, each listed 64-bit word of the (valid, live) buffer is
// read back, XORed with corrupt_xor and rewritten with plain hipMemcpy.
// Offsets outside the buffer are rejected, never accessed.
py::dict memtest(int dev, size_t bytes, const std::vector<uint64_t>& corrupt_offsets,
                 uint64_t corrupt_xor) {
    require_dev(dev);
    require(bytes >= sizeof(uint64_t), "bytes must hold at least one uint64 (8)");
    size_t n = bytes / sizeof(uint64_t);
    for (uint64_t off : corrupt_offsets)
        require(off < n, "corrupt_offsets entry is outside the buffer");
    HIP_CHECK(hipSetDevice(dev));
    DevBuf buf_mem(n * sizeof(uint64_t));
    uint64_t* buf = buf_mem.as<uint64_t>();
    uint64_t mismatches = pattern_mismatches(buf, buf, n, compute_units(dev) * 8, [&] {
        if (corrupt_offsets.empty()) return;
        HIP_CHECK(hipDeviceSynchronize());
        for (uint64_t off : corrupt_offsets) {
            uint64_t w = 0;
            HIP_CHECK(hipMemcpy(&w, buf + off, sizeof(w), hipMemcpyDeviceToHost));
            w ^= corrupt_xor;
            HIP_CHECK(hipMemcpy(buf + off, &w, sizeof(w), hipMemcpyHostToDevice));
        }
    });
    py::dict d;
    d["bytes"] = (uint64_t)(n * sizeof(uint64_t));
    d["mismatches"] = mismatches;
    return d;
}

// --- probe inputs --------------------------------------------------------------

// Deterministic full-mantissa test value: random sign, 23 random mantissa
// bits, exponent in [-4, 3].
float lcg_f32(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    uint32_t u = (uint32_t)(s >> 63) << 31 |
                 (uint32_t)(123 + ((s >> 33) & 7)) << 23 |
                 (uint32_t)((s >> 40) & 0x7fffff);
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

uint16_t bf16_round_bits(float x) {
    // bf16 storage rounding (round-to-nearest-even on the top 16 bits)
    uint32_t u;
    std::memcpy(&u, &x, 4);
    uint32_t lsb = (u >> 16) & 1u;
    u += 0x7fffu + lsb;
    return (uint16_t)(u >> 16);
}

float bf16_bits_to_float(uint16_t h) {
    uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

// The f32 probe's fixed tile: A (16×4), B (4×16) and the host's product.
void f32_probe_tile(std::vector<float>& hA, std::vector<float>& hB,
                    std::vector<float>& ref) {
    hA.assign(16 * 4, 0.f);
    hB.assign(4 * 16, 0.f);
    ref.assign(16 * 16, 0.f);
    // Full-mantissa inputs over 8 binades: products and partial sums round at
    // every step, so only the documented k-ordered fmaf chain reproduces the
    // bits (dyadic inputs would pass under any order or internal width).
    uint64_t rng = 0x243F6A8885A308D3ull;
    for (float& v : hA) v = lcg_f32(rng);
    for (float& v : hB) v = lcg_f32(rng);
    for (int i = 0; i < 16; i++)
        for (int j = 0; j < 16; j++)
            for (int k = 0; k < 4; k++)
                ref[i * 16 + j] = fmaf(hA[i * 4 + k], hB[k * 16 + j], ref[i * 16 + j]);
}

// The bf16 probe's fixed tile inputs, as bf16 bit patterns: A (32×16) and
// B (16×32), random values over 8 binades (all 8 significand bits in play).
void bf16_probe_inputs(std::vector<uint16_t>& hA, std::vector<uint16_t>& hB) {
    uint64_t rng = 0x13198A2E03707344ull;
    hA.assign(32 * 16, 0);
    hB.assign(16 * 32, 0);
    for (uint16_t& v : hA) v = bf16_round_bits(lcg_f32(rng));
    for (uint16_t& v : hB) v = bf16_round_bits(lcg_f32(rng));
}

// Host decoders for the low-precision reference (finite codes only).
double decode_fp8(uint8_t c, int ebits) {
    int mbits = 7 - ebits, bias = (1 << (ebits - 1)) - 1;
    int e = (c >> mbits) & ((1 << ebits) - 1), m = c & ((1 << mbits) - 1);
    double v = e ? std::ldexp(1.0 + m / (double)(1 << mbits), e - bias)
                 : std::ldexp(m / (double)(1 << mbits), 1 - bias);
    return (c & 0x80) ? -v : v;
}

double decode_e2m1(uint8_t c) {
    static const double mag[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
    return (c & 8) ? -mag[c & 7] : mag[c & 7];
}

double decode_code(uint8_t c, int fmt) {
    return fmt == FMT_E2M1 ? decode_e2m1(c) : decode_fp8(c, fmt == FMT_E4M3 ? 4 : 5);
}

// Exact-tile operand code: e4m3 with random sign and mantissa and exponent
// field 6..9 (|v| in [0.5, 7.5], step 2^-4 at the least), or any e2m1 code.
uint8_t exact_code(uint64_t& rng, int fmt) {
    uint32_t r = lcg_bits(rng);
    if (fmt == FMT_E2M1) return (uint8_t)(r & 15);
    return (uint8_t)((r & 0x87) | (6 + ((r >> 8) & 3)) << 3);
}

struct LowpOperands {
    std::vector<uint8_t> A, B, SA, SB;   // codes (16×K, K×16) and E8M0 scales
    std::vector<float> ref;              // the host's 16×16 product
};

constexpr uint64_t LOWP_SEED_FP8 = 0xA4093822299F31D0ull;
constexpr uint64_t LOWP_SEED_MX_FP8 = 0x082EFA98EC4E6C89ull;
constexpr uint64_t LOWP_SEED_MX_FP4 = 0x452821E638D01377ull;

// The fixed exact tile of one format: MX (K = 128, random scales 127..128 for
// e4m3, 125..129 for e2m1) or non-scaled fp8 (K = 32).
// Every product and partial sum is a multiple of the smallest product step q
// and Σ|a·b| < 2^24·q — e4m3: q = 2^-8, Σ ≤ 128·(7.5·2)^2 = 2^14.8 = 2^22.8·q;
// e2m1: q = 2^-6, Σ ≤ 128·(6·4)^2 = 2^16.2 = 2^22.2·q — so the fp64 product
// cast to f32 is the answer under any summation order: the comparison is
// bitwise, no tolerance.
LowpOperands lowp_exact_operands(int fmt, bool mx, uint64_t seed) {
    const int K = mx ? 128 : 32, NB = K / 32;
    const int s_lo = fmt == FMT_E2M1 ? 125 : 127, s_n = fmt == FMT_E2M1 ? 5 : 2;
    LowpOperands op;
    op.A.assign(16 * 128, 0);
    op.B.assign(128 * 16, 0);
    op.SA.assign(64, 127);
    op.SB.assign(64, 127);
    std::vector<uint8_t>&A = op.A, &B = op.B, &SA = op.SA, &SB = op.SB;
    uint64_t rng = seed;
    for (int i = 0; i < 16 * K; i++) A[i] = exact_code(rng, fmt);
    for (int i = 0; i < K * 16; i++) B[i] = exact_code(rng, fmt);
    if (mx) {
        for (uint8_t& s : SA) s = (uint8_t)(s_lo + lcg_bits(rng) % s_n);
        for (uint8_t& s : SB) s = (uint8_t)(s_lo + lcg_bits(rng) % s_n);
    }
    op.ref.assign(256, 0.f);
    for (int i = 0; i < 16; i++)
        for (int j = 0; j < 16; j++) {
            double sum = 0;
            for (int b = 0; b < NB; b++) {
                double part = 0;
                for (int k = 32 * b; k < 32 * b + 32; k++)
                    part += decode_code(A[i * K + k], fmt) * decode_code(B[k * 16 + j], fmt);
                sum += std::ldexp(part, SA[i * 4 + b] - 127 + SB[b * 16 + j] - 127);
            }
            op.ref[i * 16 + j] = (float)sum;
        }
    return op;
}

// --- f32 / bf16 ----------------------------------------------------------------

// One launch of mfma_f32_tile on `blocks` blocks → blocks × 256 floats.
// C may be nullptr (zero accumulator).
std::vector<float> run_f32_tile(const float* A, const float* B, const float* C,
                                int blocks) {
    DevBuf dA = upload(A, 64 * 4), dB = upload(B, 64 * 4), dC(256 * 4);
    if (C) HIP_CHECK(hipMemcpy(dC.p, C, 256 * 4, hipMemcpyHostToDevice));
    return launch_fetch((size_t)blocks * 256, [&](float* dD) {
        hipLaunchKernelGGL(mfma_f32_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<float>(), dB.as<float>(),
                           C ? dC.as<float>() : (const float*)nullptr, dD);
    });
}

py::bytes mfma_f32_tile_run(int dev, py::buffer A, py::buffer B, py::object C,
                            int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A.request(), ib = B.request();
    const float* pa = (const float*)tile_buffer(ia, 4, 64, "A must be 16x4 contiguous f32");
    const float* pb = (const float*)tile_buffer(ib, 4, 64, "B must be 4x16 contiguous f32");
    py::buffer_info ic;
    const float* pc = nullptr;
    if (!C.is_none()) {
        ic = py::cast<py::buffer>(C).request();
        pc = (const float*)tile_buffer(ic, 4, 256, "C must be 16x16 contiguous f32");
    }
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_f32_tile(pa, pb, pc, blocks));
}

py::dict mfma_probe_f32(int dev) {
    require_dev(dev);
    HIP_CHECK(hipSetDevice(dev));
    std::vector<float> hA, hB, ref;
    f32_probe_tile(hA, hB, ref);
    // 2 blocks per CU: every CU's matrix cores run the tile
    int blocks = std::min(compute_units(dev) * 2, MAX_TILE_BLOCKS);
    std::vector<float> hD = run_f32_tile(hA.data(), hB.data(), nullptr, blocks);
    double max_abs_err = 0;
    for (int i = 0; i < 256; i++) {
        double e = std::fabs((double)hD[i] - (double)ref[i]);
        if (std::isnan(e)) { max_abs_err = e; break; }   // std::max would drop it
        max_abs_err = std::max(max_abs_err, e);
    }
    bool bits_equal = std::memcmp(hD.data(), ref.data(), 256 * 4) == 0;
    uint64_t bad_slabs = slab_mismatches(hD, 256);
    py::dict d;
    d["max_abs_err"] = max_abs_err;   // exact f32 MFMA ⇒ expect 0.0
    d["slab_mismatches"] = bad_slabs;
    d["blocks"] = blocks;
    d["ok"] = bits_equal && bad_slabs == 0;
    return d;
}

// One launch of mfma_bf16_tile on `blocks` blocks → blocks × 1024 floats.
std::vector<float> run_bf16_tile(const uint16_t* A, const uint16_t* B, int blocks) {
    DevBuf dA = upload(A, 512 * 2), dB = upload(B, 512 * 2);
    return launch_fetch((size_t)blocks * 1024, [&](float* dD) {
        hipLaunchKernelGGL(mfma_bf16_tile, dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const __bf16>(), dB.as<const __bf16>(), dD);
    });
}

py::bytes mfma_bf16_tile_run(int dev, py::buffer A_bits, py::buffer B_bits, int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    py::buffer_info ia = A_bits.request(), ib = B_bits.request();
    const uint16_t* pa = (const uint16_t*)tile_buffer(
        ia, 2, 512, "A_bits must be 32x16 contiguous uint16");
    const uint16_t* pb = (const uint16_t*)tile_buffer(
        ib, 2, 512, "B_bits must be 16x32 contiguous uint16");
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_bf16_tile(pa, pb, blocks));
}

void launch_bf16_burn(int blocks, float* out, int iters) {
    hipLaunchKernelGGL(mfma_bf16_burn, dim3(blocks), dim3(256), 0, 0, out, iters);
}

py::dict mfma_bf16_burn_run(int dev, int iters, int blocks) {
    require_dev(dev);
    require(iters > 0, "iters must be > 0");
    require_burn_blocks(blocks);
    HIP_CHECK(hipSetDevice(dev));
    return raw_burn(launch_bf16_burn, burn_blocks(dev, blocks, 2), iters);
}

// Each bf16×bf16 product is exact in f32 and the 16 additions lose at most
// one ulp each in any order, so |D − ref| ≤ 16·2^-23·Σ|a·b| holds for a
// healthy matrix core whatever its internal summation order; a mapping error
// is O(1) relative. `D` is one 32×32 slab.
bool bf16_tile_within_bound(const std::vector<uint16_t>& hA,
                            const std::vector<uint16_t>& hB, const float* D,
                            double& max_rel_err) {
    bool tile_ok = true;
    max_rel_err = 0;
    for (int i = 0; i < 32; i++)
        for (int j = 0; j < 32; j++) {
            double ref = 0, mag = 0;
            for (int k = 0; k < 16; k++) {
                double p = (double)bf16_bits_to_float(hA[i * 16 + k]) *
                           (double)bf16_bits_to_float(hB[k * 32 + j]);
                ref += p;
                mag += std::fabs(p);
            }
            double err = std::fabs((double)D[i * 32 + j] - ref);
            if (!(err <= 16.0 * 0x1p-23 * mag)) tile_ok = false;   // NaN fails
            if (!std::isnan(max_rel_err)) {
                double rel = err / std::max(1.0, std::fabs(ref));
                max_rel_err = std::isnan(rel) ? rel : std::max(max_rel_err, rel);
            }
        }
    return tile_ok;
}

py::dict mfma_probe_bf16(int dev, int burn_iters) {
    require_dev(dev);
    require(burn_iters > 0, "burn_iters must be > 0");
    HIP_CHECK(hipSetDevice(dev));
    // --- correctness tile ---
    std::vector<uint16_t> hA, hB;
    bf16_probe_inputs(hA, hB);
    int blocks = std::min(compute_units(dev) * 2, MAX_TILE_BLOCKS);
    std::vector<float> hD = run_bf16_tile(hA.data(), hB.data(), blocks);
    double max_rel_err = 0;
    bool tile_ok = bf16_tile_within_bound(hA, hB, hD.data(), max_rel_err);
    uint64_t bad_slabs = slab_mismatches(hD, 1024);

    // --- throughput burn: 2 × 256-thread WGs per CU, so it covers every CU ---
    // FLOPs per block and iteration: 4 waves/WG × 4 acc × 2·32·32·16
    TimedBurn burn = timed_burn(launch_bf16_burn, burn_blocks(dev, 0, 2), burn_iters,
                                4.0 * 4.0 * 2.0 * 32 * 32 * 16);
    py::dict d;
    d["max_rel_err"] = max_rel_err;
    d["slab_mismatches"] = bad_slabs;
    d["burn_mismatches"] = burn.mismatches;
    d["ok"] = tile_ok && bad_slabs == 0;
    d["tflops"] = burn.tflops;
    d["burn_ms"] = burn.ms;
    return d;
}

// --- FP8 / MX -----------------------------------------------------------------

using fp8_kernel_t = void (*)(const uint8_t*, const uint8_t*, float*);
using mx_kernel_t = void (*)(const uint8_t*, const uint8_t*, const uint8_t*,
                             const uint8_t*, float*);

fp8_kernel_t fp8_kernel(int af, int bf) {
    if (af == FMT_E4M3) return bf == FMT_E4M3 ? mfma_fp8_tile<FMT_E4M3, FMT_E4M3>
                                              : mfma_fp8_tile<FMT_E4M3, FMT_E5M2>;
    return bf == FMT_E4M3 ? mfma_fp8_tile<FMT_E5M2, FMT_E4M3>
                          : mfma_fp8_tile<FMT_E5M2, FMT_E5M2>;
}

// cbsz and blgp are immediates, so each format pair is its own kernel.
template <int AF>
mx_kernel_t mx_kernel_b(int bf) {
    switch (bf) {
        case FMT_E4M3: return mfma_mx_tile<AF, FMT_E4M3>;
        case FMT_E5M2: return mfma_mx_tile<AF, FMT_E5M2>;
        default:       return mfma_mx_tile<AF, FMT_E2M1>;
    }
}

mx_kernel_t mx_kernel(int af, int bf) {
    switch (af) {
        case FMT_E4M3: return mx_kernel_b<FMT_E4M3>(bf);
        case FMT_E5M2: return mx_kernel_b<FMT_E5M2>(bf);
        default:       return mx_kernel_b<FMT_E2M1>(bf);
    }
}

// One launch of mfma_fp8_tile on `blocks` blocks → blocks × 256 floats.
std::vector<float> run_fp8_tile(const uint8_t* A, const uint8_t* B, int af, int bf,
                                int blocks) {
    DevBuf dA = upload(A, 512), dB = upload(B, 512);
    return launch_fetch((size_t)blocks * 256, [&](float* dD) {
        hipLaunchKernelGGL(fp8_kernel(af, bf), dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const uint8_t>(), dB.as<const uint8_t>(), dD);
    });
}

// One launch of mfma_mx_tile on `blocks` blocks → blocks × 256 floats.
std::vector<float> run_mx_tile(const uint8_t* A, const uint8_t* B, const uint8_t* SA,
                               const uint8_t* SB, int af, int bf, int blocks) {
    DevBuf dA = upload(A, 2048), dB = upload(B, 2048), dSA = upload(SA, 64),
           dSB = upload(SB, 64);
    return launch_fetch((size_t)blocks * 256, [&](float* dD) {
        hipLaunchKernelGGL(mx_kernel(af, bf), dim3(blocks), dim3(WAVE), 0, 0,
                           dA.as<const uint8_t>(), dB.as<const uint8_t>(),
                           dSA.as<const uint8_t>(), dSB.as<const uint8_t>(), dD);
    });
}

py::bytes mfma_fp8_tile_run(int dev, py::buffer A_codes, py::buffer B_codes,
                            const std::string& a_fmt, const std::string& b_fmt,
                            int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    int af = parse_fmt(a_fmt, {FMT_E4M3, FMT_E5M2}, "a_fmt must be 'e4m3' or 'e5m2'");
    int bf = parse_fmt(b_fmt, {FMT_E4M3, FMT_E5M2}, "b_fmt must be 'e4m3' or 'e5m2'");
    py::buffer_info ia = A_codes.request(), ib = B_codes.request();
    const uint8_t* pa = typed_buffer<uint8_t>(ia, 512, "A_codes must be 16x32 contiguous uint8");
    const uint8_t* pb = typed_buffer<uint8_t>(ib, 512, "B_codes must be 32x16 contiguous uint8");
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_fp8_tile(pa, pb, af, bf, blocks));
}

py::bytes mfma_mx_tile_run(int dev, py::buffer A_codes, py::buffer B_codes,
                           py::buffer A_scales, py::buffer B_scales,
                           const std::string& a_fmt, const std::string& b_fmt,
                           int blocks) {
    require_dev(dev);
    require_tile_blocks(blocks);
    int af = parse_fmt(a_fmt, {FMT_E4M3, FMT_E5M2, FMT_E2M1},
                       "a_fmt must be 'e4m3', 'e5m2' or 'e2m1'");
    int bf = parse_fmt(b_fmt, {FMT_E4M3, FMT_E5M2, FMT_E2M1},
                       "b_fmt must be 'e4m3', 'e5m2' or 'e2m1'");
    py::buffer_info ia = A_codes.request(), ib = B_codes.request();
    py::buffer_info isa = A_scales.request(), isb = B_scales.request();
    const uint8_t* pa = typed_buffer<uint8_t>(ia, 2048, "A_codes must be 16x128 contiguous uint8");
    const uint8_t* pb = typed_buffer<uint8_t>(ib, 2048, "B_codes must be 128x16 contiguous uint8");
    const uint8_t* psa = typed_buffer<uint8_t>(isa, 64, "A_scales must be 16x4 contiguous uint8");
    const uint8_t* psb = typed_buffer<uint8_t>(isb, 64, "B_scales must be 4x16 contiguous uint8");
    for (int i = 0; i < 2048; i++) {
        require(af != FMT_E2M1 || pa[i] < 16, "A_codes: an e2m1 code must be below 16");
        require(bf != FMT_E2M1 || pb[i] < 16, "B_codes: an e2m1 code must be below 16");
    }
    HIP_CHECK(hipSetDevice(dev));
    return as_bytes(run_mx_tile(pa, pb, psa, psb, af, bf, blocks));
}

void launch_mx_burn(int fmt, int blocks, float* out, int iters) {
    if (fmt == FMT_E2M1)
        hipLaunchKernelGGL(mfma_mx_burn<FMT_E2M1>, dim3(blocks), dim3(256), 0, 0, out, iters);
    else
        hipLaunchKernelGGL(mfma_mx_burn<FMT_E4M3>, dim3(blocks), dim3(256), 0, 0, out, iters);
}

// launch_mx_burn of one format, in the burns' launcher shape.
auto mx_burn_launcher(int fmt) {
    return [fmt](int blocks, float* out, int iters) { launch_mx_burn(fmt, blocks, out, iters); };
}

py::dict mfma_mx_burn_run(int dev, const std::string& fmt, int iters, int blocks) {
    require_dev(dev);
    int f = parse_fmt(fmt, {FMT_E4M3, FMT_E2M1}, "fmt must be 'e4m3' or 'e2m1'");
    require(iters > 0, "iters must be > 0");
    require_burn_blocks(blocks);
    HIP_CHECK(hipSetDevice(dev));
    return raw_burn(mx_burn_launcher(f), burn_blocks(dev, blocks, 2), iters);
}

// The exact tile of lowp_exact_operands on `blocks` blocks: slab 0 against the
// host, every other slab against slab 0.
TileVerdict lowp_exact_tile(int fmt, bool mx, int blocks, uint64_t seed) {
    LowpOperands op = lowp_exact_operands(fmt, mx, seed);
    std::vector<float> hD = mx
        ? run_mx_tile(op.A.data(), op.B.data(), op.SA.data(), op.SB.data(), fmt, fmt, blocks)
        : run_fp8_tile(op.A.data(), op.B.data(), fmt, fmt, blocks);
    return judge_tile(hD, op.ref);
}

// FP8 / MX-FP8 / MX-FP4 matrix-core probe: one fixed exact tile per form on
// 2 blocks per CU (slab 0 bitwise against the host's fp64 product, every
// other slab bitwise against slab 0), then a timed MX-fp8 and MX-fp4 burn,
// each after a warm-up launch, whose waves must all agree bit for bit.
// If a burn rate falls short of the guide's peak (~5 PF MX-fp8, ~10 PF
// MX-fp4), the things to revisit are the accumulator count (MX_BURN_ACCS = 8),
// the waves per SIMD (2: two 256-thread workgroups per CU) and the shape
// (16x16x128; the 32x32x64 form moves half the operand bytes per FLOP).
// FP6 operands are not probed: same datapath and rate as FP4.
py::dict mfma_probe_lowp(int dev, int burn_iters) {
    require_dev(dev);
    require(burn_iters > 0, "burn_iters must be > 0");
    HIP_CHECK(hipSetDevice(dev));
    int blocks = std::min(compute_units(dev) * 2, MAX_TILE_BLOCKS);
    TileVerdict fp8 = lowp_exact_tile(FMT_E4M3, false, blocks, LOWP_SEED_FP8);
    TileVerdict mx8 = lowp_exact_tile(FMT_E4M3, true, blocks, LOWP_SEED_MX_FP8);
    TileVerdict mx4 = lowp_exact_tile(FMT_E2M1, true, blocks, LOWP_SEED_MX_FP4);
    int burn_grid = burn_blocks(dev, 0, 2);   // 2 × 256-thread WGs per CU
    // FLOPs per block and iteration: 4 waves/WG × accumulators × 2·16·16·128
    const double burn_flops = 4.0 * MX_BURN_ACCS * 2.0 * 16 * 16 * 128;
    TimedBurn b8 = timed_burn(mx_burn_launcher(FMT_E4M3), burn_grid, burn_iters, burn_flops);
    TimedBurn b4 = timed_burn(mx_burn_launcher(FMT_E2M1), burn_grid, burn_iters, burn_flops);
    py::dict d;
    d["fp8_ok"] = fp8.ok;
    d["mx_fp8_ok"] = mx8.ok;
    d["mx_fp4_ok"] = mx4.ok;
    d["fp8_slab_mismatches"] = fp8.bad_slabs;
    d["mx_fp8_slab_mismatches"] = mx8.bad_slabs;
    d["mx_fp4_slab_mismatches"] = mx4.bad_slabs;
    d["mx_fp8_tflops"] = b8.tflops;
    d["mx_fp4_tflops"] = b4.tflops;
    d["mx_fp8_burn_mismatches"] = b8.mismatches;
    d["mx_fp4_burn_mismatches"] = b4.mismatches;
    d["mx_fp8_burn_ms"] = b8.ms;
    d["mx_fp4_burn_ms"] = b4.ms;
    d["blocks"] = blocks;
    return d;
}

// --- unit sweep -----------------------------------------------------------------

const char* const SWEEP_KIND_NAMES[SK_COUNT] = {"f32", "bf16", "fp8", "mx_fp8", "mx_fp4", "lds"};

constexpr int SWEEP_MAX_REPS = 1 << 20;
constexpr int SWEEP_MAX_BLOCKS = 4096;
// Measured on MI355X (profiles/unit_sweep.md): the four waves of a 256-thread
// workgroup sit on four SIMDs, and with the LDS check in the launch one
// repetition already covered all 1024 SIMDs in a first launch, three runs of
// three; the default is that smallest count doubled once.
constexpr int SWEEP_THREADS = 256;
constexpr int SWEEP_DEFAULT_REPS = 2;
constexpr int SWEEP_MAX_LAUNCHES = 3;
constexpr size_t SWEEP_LDS_GRANULE = 4096;   // a multiple of 4 × the largest block

void require_sweep_reps(int reps) {
    require(reps >= 1 && reps <= SWEEP_MAX_REPS, "reps must be in 1..2^20");
}

int sweep_kind(const std::string& s, const char* what) {
    for (int k = 0; k < SK_COUNT; k++)
        if (s == SWEEP_KIND_NAMES[k]) return k;
    throw std::invalid_argument(what);
}

uint32_t sweep_kind_mask(const std::vector<std::string>& kinds) {
    require(!kinds.empty(), "kinds must not be empty");
    uint32_t mask = 0;
    for (const std::string& s : kinds)
        mask |= 1u << sweep_kind(
            s, "kinds must be among 'f32', 'bf16', 'fp8', 'mx_fp8', 'mx_fp4', 'lds'");
    return mask;
}

// poison = (xcc_id, cu_key, simd_id, kind, xor_bits) or None → SweepParams.
void sweep_parse_poison(const py::object& poison, uint32_t kinds, SweepParams& p) {
    p.poison_kind = -1;
    p.poison_xcc = p.poison_cu_key = p.poison_simd = p.poison_xor = 0;
    if (poison.is_none()) return;
    long long xcc, cu, simd, bits;
    std::string kind;
    require(py::isinstance<py::tuple>(poison) || py::isinstance<py::list>(poison),
            "poison must be (xcc_id, cu_key, simd_id, kind, xor_bits)");
    try {
        py::tuple t = py::cast<py::tuple>(poison);
        require(t.size() == 5, "poison must be (xcc_id, cu_key, simd_id, kind, xor_bits)");
        xcc = py::cast<long long>(t[0]);
        cu = py::cast<long long>(t[1]);
        simd = py::cast<long long>(t[2]);
        kind = py::cast<std::string>(t[3]);
        bits = py::cast<long long>(t[4]);
    } catch (const py::cast_error&) {
        throw std::invalid_argument("poison must be (xcc_id, cu_key, simd_id, kind, xor_bits)");
    }
    require(xcc >= 0 && xcc <= 15, "poison xcc_id must be in 0..15");
    require(cu >= 0 && cu <= 255, "poison cu_key must be in 0..255");
    require(simd >= 0 && simd <= 3, "poison simd_id must be in 0..3");
    p.poison_kind = sweep_kind(kind, "poison kind must be one of the six kind names");
    require(kinds >> p.poison_kind & 1, "poison kind must be among the selected kinds");
    require(bits >= 1 && bits <= 0xffffffffll, "poison xor_bits must be in 1..2^32-1");
    p.poison_xcc = (uint32_t)xcc;
    p.poison_cu_key = (uint32_t)cu;
    p.poison_simd = (uint32_t)simd;
    p.poison_xor = (uint32_t)bits;
}

// Inputs and golden tiles of the selected kinds. f32, fp8, MX-fp8 and MX-fp4
// are the host references of mfma_probe_f32 and mfma_probe_lowp; bf16 has no
// bitwise host reference, so its golden tile is a one-block mfma_bf16_tile
// launch that passed the probe's tolerance check (else golden_ok[bf16] = false
// and the kind is dropped from the sweep).
struct SweepSetup {
    SweepInputs in;
    uint32_t kinds;                 // what will run
    bool golden_ok[SK_COUNT];
};

void sweep_prepare(uint32_t kinds, SweepSetup& s) {
    std::memset(&s.in, 0, sizeof(s.in));
    s.kinds = kinds;
    for (bool& ok : s.golden_ok) ok = true;
    if (kinds & (1u << SK_F32)) {
        std::vector<float> a, b, ref;
        f32_probe_tile(a, b, ref);
        std::memcpy(s.in.a32, a.data(), sizeof(s.in.a32));
        std::memcpy(s.in.b32, b.data(), sizeof(s.in.b32));
        std::memcpy(s.in.g32, ref.data(), sizeof(s.in.g32));
    }
    if (kinds & (1u << SK_BF16)) {
        std::vector<uint16_t> a, b;
        bf16_probe_inputs(a, b);
        std::vector<float> d = run_bf16_tile(a.data(), b.data(), 1);
        double max_rel_err = 0;
        if (bf16_tile_within_bound(a, b, d.data(), max_rel_err)) {
            std::memcpy(s.in.a16, a.data(), sizeof(s.in.a16));
            std::memcpy(s.in.b16, b.data(), sizeof(s.in.b16));
            std::memcpy(s.in.g16, d.data(), sizeof(s.in.g16));
        } else {
            s.golden_ok[SK_BF16] = false;
            s.kinds &= ~(1u << SK_BF16);
        }
    }
    if (kinds & (1u << SK_FP8)) {
        LowpOperands op = lowp_exact_operands(FMT_E4M3, false, LOWP_SEED_FP8);
        std::memcpy(s.in.a8, op.A.data(), sizeof(s.in.a8));
        std::memcpy(s.in.b8, op.B.data(), sizeof(s.in.b8));
        std::memcpy(s.in.g8, op.ref.data(), sizeof(s.in.g8));
    }
    if (kinds & (1u << SK_MX_FP8)) {
        LowpOperands op = lowp_exact_operands(FMT_E4M3, true, LOWP_SEED_MX_FP8);
        std::memcpy(s.in.amx8, op.A.data(), sizeof(s.in.amx8));
        std::memcpy(s.in.bmx8, op.B.data(), sizeof(s.in.bmx8));
        std::memcpy(s.in.samx8, op.SA.data(), sizeof(s.in.samx8));
        std::memcpy(s.in.sbmx8, op.SB.data(), sizeof(s.in.sbmx8));
        std::memcpy(s.in.gmx8, op.ref.data(), sizeof(s.in.gmx8));
    }
    if (kinds & (1u << SK_MX_FP4)) {
        LowpOperands op = lowp_exact_operands(FMT_E2M1, true, LOWP_SEED_MX_FP4);
        std::memcpy(s.in.amx4, op.A.data(), sizeof(s.in.amx4));
        std::memcpy(s.in.bmx4, op.B.data(), sizeof(s.in.bmx4));
        std::memcpy(s.in.samx4, op.SA.data(), sizeof(s.in.samx4));
        std::memcpy(s.in.sbmx4, op.SB.data(), sizeof(s.in.sbmx4));
        std::memcpy(s.in.gmx4, op.ref.data(), sizeof(s.in.gmx4));
    }
}

struct SweepLaunch {
    std::vector<uint32_t> records;
    int blocks = 0, waves_per_block = 0;
    size_t lds_bytes = 0;
    bool exclusive = false;
    float ms = 0;
};

// The largest LDS allocation one block may ask for, capped at a whole CU's.
size_t sweep_lds_limit(int dev) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    size_t limit = std::max(prop.sharedMemPerBlock, prop.sharedMemPerBlockOptin);
    limit = std::min(limit, CU_LDS_BYTES);
    return limit / SWEEP_LDS_GRANULE * SWEEP_LDS_GRANULE;
}

// One launch of unit_sweep. More than half a CU's LDS per block makes the
// blocks exclusive; if the device grants no more than that, or refuses the
// large launch, the sweep runs on 64 KiB blocks, as many as fit the chip at
// once, with exclusive = false, and the coverage numbers speak for themselves.
SweepLaunch sweep_launch(int dev, const SweepSetup& setup, SweepParams p, int blocks_arg,
                         int threads) {
    const size_t fallback = 64 << 10;
    size_t lds = sweep_lds_limit(dev);
    require(lds >= SWEEP_LDS_GRANULE, "device reports no usable LDS");
    bool exclusive = lds > CU_LDS_BYTES / 2;
    if (exclusive && lds > fallback &&
        hipFuncSetAttribute(reinterpret_cast<const void*>(unit_sweep),
                            hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds) != hipSuccess) {
        (void)hipGetLastError();   // refused: not sticky
        lds = fallback;
        exclusive = false;
    }
    if (!exclusive) lds = std::min(lds, fallback);

    DevBuf d_in = upload(&setup.in, sizeof(SweepInputs));
    const int cus = compute_units(dev);
    SweepLaunch out;
    for (;;) {
        int blocks = blocks_arg > 0 ? blocks_arg
                                    : std::min(SWEEP_MAX_BLOCKS, cus * (int)(CU_LDS_BYTES / lds));
        int wpb = threads / WAVE;
        size_t n_words = (size_t)blocks * wpb * SWEEP_RECORD_WORDS;
        DevBuf d_rec(n_words * 4);
        // an unwritten record reads as all ones: no valid XCD, every counter bad
        HIP_CHECK(hipMemset(d_rec.p, 0xff, n_words * 4));
        p.lds_words = (uint32_t)(lds / 4);
        hipError_t launched = hipSuccess;
        out.ms = timed_ms([&] {
            hipLaunchKernelGGL(unit_sweep, dim3(blocks), dim3(threads), lds, 0,
                               d_in.as<const SweepInputs>(), p, d_rec.as<uint32_t>());
            launched = hipGetLastError();
        });
        if (launched != hipSuccess && exclusive) {
            // the large-LDS launch was refused before anything ran
            lds = fallback;
            exclusive = false;
            continue;
        }
        HIP_CHECK(launched);
        HIP_CHECK(hipDeviceSynchronize());
        out.records.resize(n_words);
        HIP_CHECK(hipMemcpy(out.records.data(), d_rec.p, n_words * 4, hipMemcpyDeviceToHost));
        out.blocks = blocks;
        out.waves_per_block = wpb;
        out.lds_bytes = lds;
        out.exclusive = exclusive;
        return out;
    }
}

py::dict sweep_golden_dict(uint32_t kinds, const SweepSetup& setup) {
    py::dict g;
    for (int k = 0; k < SK_COUNT; k++)
        if (kinds >> k & 1) g[SWEEP_KIND_NAMES[k]] = setup.golden_ok[k];
    return g;
}

// Raw entry point: one launch, no retries.
py::dict unit_sweep_run(int dev, const std::vector<std::string>& kinds, int reps, int blocks,
                        const py::object& poison, int threads) {
    require_dev(dev);
    uint32_t mask = sweep_kind_mask(kinds);
    require_sweep_reps(reps);
    require(blocks >= 0 && blocks <= SWEEP_MAX_BLOCKS, "blocks must be in 0..4096");
    require(threads == 256 || threads == 512 || threads == 1024,
            "threads must be 256, 512 or 1024");
    SweepParams p{};
    sweep_parse_poison(poison, mask, p);
    HIP_CHECK(hipSetDevice(dev));
    SweepSetup setup;
    sweep_prepare(mask, setup);
    p.kinds = setup.kinds;
    p.reps = reps;
    SweepLaunch r = sweep_launch(dev, setup, p, blocks, threads);
    py::dict d;
    d["records"] = as_bytes(r.records);
    d["waves_per_block"] = r.waves_per_block;
    d["blocks"] = r.blocks;
    d["lds_bytes_per_block"] = (uint64_t)r.lds_bytes;
    d["exclusive"] = r.exclusive;
    d["golden_ok"] = sweep_golden_dict(mask, setup);
    d["sweep_ms"] = r.ms;
    d["reps"] = reps;
    return d;
}

// Distinct (XCD, CU key, SIMD) triples in the records: HW_ID bits 15:8 are
// the CU key, bits 5:4 the SIMD, XCC_ID bits 3:0 the XCD.
size_t sweep_simds_seen(const std::vector<uint32_t>& records) {
    std::vector<uint32_t> keys;
    for (size_t i = 0; i + 1 < records.size(); i += SWEEP_RECORD_WORDS)
        keys.push_back((records[i + 1] & 15u) << 10 | (records[i] >> 8 & 255u) << 2 |
                       (records[i] >> 4 & 3u));
    std::sort(keys.begin(), keys.end());
    return std::unique(keys.begin(), keys.end()) - keys.begin();
}

// What probe_device calls: the sweep, launched again (three launches at most)
// only while the merged records do not cover 4 SIMDs on every CU. A HIP error
// propagates; nothing is relaunched after one.
py::dict unit_sweep_probe(int dev, bool low_precision, int reps) {
    require_dev(dev);
    require_sweep_reps(reps);
    uint32_t mask = 1u << SK_F32 | 1u << SK_BF16 | 1u << SK_LDS;
    if (low_precision) mask |= 1u << SK_FP8 | 1u << SK_MX_FP8 | 1u << SK_MX_FP4;
    HIP_CHECK(hipSetDevice(dev));
    SweepSetup setup;
    sweep_prepare(mask, setup);
    SweepParams p{};
    p.poison_kind = -1;
    p.kinds = setup.kinds;
    p.reps = reps;
    const size_t expected = (size_t)compute_units(dev) * 4;
    std::vector<uint32_t> merged;
    SweepLaunch last;
    float total_ms = 0;
    int launches = 0;
    bool exclusive = true;
    while (launches < SWEEP_MAX_LAUNCHES) {
        last = sweep_launch(dev, setup, p, 0, SWEEP_THREADS);
        launches++;
        total_ms += last.ms;
        exclusive = exclusive && last.exclusive;
        merged.insert(merged.end(), last.records.begin(), last.records.end());
        if (sweep_simds_seen(merged) >= expected) break;
    }
    py::dict d;
    d["records"] = as_bytes(merged);
    d["waves_per_block"] = last.waves_per_block;
    d["blocks"] = last.blocks;
    d["lds_bytes_per_block"] = (uint64_t)last.lds_bytes;
    d["exclusive"] = exclusive;
    d["golden_ok"] = sweep_golden_dict(mask, setup);
    d["sweep_ms"] = total_ms;
    d["reps"] = reps;
    d["launches"] = launches;
    return d;
}

}  // namespace

PYBIND11_MODULE(_gpuprobe, m) {
    m.doc() = "MI355X (gfx950) health/burn-in probes for kata-xpu-device-plugin-amd";
    m.def("device_count", &device_count);
    m.def("device_info", &device_info, py::arg("dev") = 0);
    m.def("hbm_bandwidth_probe", &hbm_bandwidth_probe, py::arg("dev") = 0,
          py::arg("bytes") = (size_t)1 << 31, py::arg("iters") = 5);
    m.def("memtest", &memtest, py::arg("dev") = 0, py::arg("bytes") = (size_t)1 << 31,
          py::arg("corrupt_offsets") = std::vector<uint64_t>{},
          py::arg("corrupt_xor") = (uint64_t)1);
    m.def("hbm_copy_check", &hbm_copy_check, py::arg("dev") = 0,
          py::arg("bytes") = (size_t)1 << 28);
    m.def("lds_read_burn_run", &lds_read_burn_run, py::arg("dev") = 0,
          py::arg("iters") = 256, py::arg("blocks") = 0);
    m.def("mfma_f32_tile_run", &mfma_f32_tile_run, py::arg("dev"), py::arg("A"),
          py::arg("B"), py::arg("C") = py::none(), py::arg("blocks") = 1);
    m.def("mfma_bf16_tile_run", &mfma_bf16_tile_run, py::arg("dev"),
          py::arg("A_bits"), py::arg("B_bits"), py::arg("blocks") = 1);
    m.def("mfma_bf16_burn_run", &mfma_bf16_burn_run, py::arg("dev") = 0,
          py::arg("iters") = 64, py::arg("blocks") = 0);
    m.def("pcie_bandwidth_probe", &pcie_bandwidth_probe, py::arg("dev") = 0,
          py::arg("bytes") = (size_t)256 << 20, py::arg("iters") = 5);
    m.def("lds_bandwidth_probe", &lds_bandwidth_probe, py::arg("dev") = 0,
          py::arg("iters") = 100000);
    m.def("hbm_latency_probe", &hbm_latency_probe, py::arg("dev") = 0,
          py::arg("bytes") = (size_t)1 << 30, py::arg("steps") = 2000000);
    m.def("mfma_probe_f32", &mfma_probe_f32, py::arg("dev") = 0);
    m.def("mfma_probe_bf16", &mfma_probe_bf16, py::arg("dev") = 0,
          py::arg("burn_iters") = 20000);
    m.def("mfma_fp8_tile_run", &mfma_fp8_tile_run, py::arg("dev"), py::arg("A_codes"),
          py::arg("B_codes"), py::arg("a_fmt"), py::arg("b_fmt"), py::arg("blocks") = 1);
    m.def("mfma_mx_tile_run", &mfma_mx_tile_run, py::arg("dev"), py::arg("A_codes"),
          py::arg("B_codes"), py::arg("A_scales"), py::arg("B_scales"),
          py::arg("a_fmt"), py::arg("b_fmt"), py::arg("blocks") = 1);
    m.def("mfma_mx_burn_run", &mfma_mx_burn_run, py::arg("dev"), py::arg("fmt"),
          py::arg("iters") = 64, py::arg("blocks") = 0);
    m.def("mfma_probe_lowp", &mfma_probe_lowp, py::arg("dev") = 0,
          py::arg("burn_iters") = 20000);
    m.def("unit_sweep_run", &unit_sweep_run, py::arg("dev"), py::arg("kinds"),
          py::arg("reps"), py::arg("blocks") = 0, py::arg("poison") = py::none(),
          py::arg("threads") = SWEEP_THREADS);
    m.def("unit_sweep_probe", &unit_sweep_probe, py::arg("dev") = 0,
          py::arg("low_precision") = false, py::arg("reps") = SWEEP_DEFAULT_REPS);
    m.attr("UNIT_SWEEP_DEFAULT_REPS") = SWEEP_DEFAULT_REPS;
}
