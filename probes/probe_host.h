// Host-side helpers shared by the probe extensions (xpu_probe.hip →
// _gpuprobe, xpu_probe_formats.hip → _gpuprobe_formats): argument checks,
// RAII device/host/event handles, the one launch, fetch and timing path, the
// slab / tile / burn comparisons and the tiles' bit generator. Everything has
// internal linkage; each extension is one translation unit. The device side
// both share is mfma_forms.h.
#pragma once

#include <hip/hip_runtime.h>
#include <pybind11/pybind11.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace py = pybind11;

#define HIP_CHECK(expr)                                                       \
    do {                                                                      \
        hipError_t _e = (expr);                                               \
        if (_e != hipSuccess)                                                 \
            throw std::runtime_error(std::string(#expr) + " failed: " +       \
                                     hipGetErrorString(_e));                  \
    } while (0)

namespace {

constexpr int WAVE = 64;

// Argument checks run before the first HIP call of every entry point, so a
// bad argument is a ValueError on any machine, with or without a GPU.
inline void require(bool cond, const char* what) {
    if (!cond) throw std::invalid_argument(what);
}

inline void require_dev(int dev) { require(dev >= 0, "dev must be >= 0"); }

constexpr int MAX_TILE_BLOCKS = 4096;   // 16 MiB of bf16-tile slabs at most
constexpr int MAX_BURN_BLOCKS = 65536;  // 64 MiB of burn output at most

inline void require_tile_blocks(int blocks) {
    require(blocks >= 1 && blocks <= MAX_TILE_BLOCKS, "blocks out of range");
}

// 0 asks for the entry point's own per-CU default (burn_blocks).
inline void require_burn_blocks(int blocks) {
    require(blocks >= 0 && blocks <= MAX_BURN_BLOCKS, "blocks out of range");
}

// Device memory, pinned host memory and events that are released on every
// path, exceptions included.
struct DevBuf {
    void* p = nullptr;
    explicit DevBuf(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes)); }
    ~DevBuf() { if (p) (void)hipFree(p); }
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct HostBuf {
    void* p = nullptr;
    explicit HostBuf(size_t bytes) { HIP_CHECK(hipHostMalloc(&p, bytes)); }
    ~HostBuf() { if (p) (void)hipHostFree(p); }
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
};

struct Event {
    hipEvent_t e = nullptr;
    Event() { HIP_CHECK(hipEventCreate(&e)); }
    ~Event() { if (e) (void)hipEventDestroy(e); }
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
};

// A device copy of `bytes` bytes at `src`.
inline DevBuf upload(const void* src, size_t bytes) {
    DevBuf d(bytes);
    HIP_CHECK(hipMemcpy(d.p, src, bytes, hipMemcpyHostToDevice));
    return d;
}

// Milliseconds the device spent on what `enqueue` puts on the null stream:
// one kernel launch or one async copy, and nothing else. A refused launch is
// reported once the closing event is recorded, outside the timed window.
template <class F>
float timed_ms(F&& enqueue) {
    Event t0, t1;
    HIP_CHECK(hipEventRecord(t0.e));
    enqueue();
    HIP_CHECK(hipEventRecord(t1.e));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventSynchronize(t1.e));
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, t0.e, t1.e));
    return ms;
}

template <class F>
float best_timed_ms(int iters, F&& enqueue) {
    float best = 1e30f;
    for (int i = 0; i < iters; i++) best = std::min(best, timed_ms(enqueue));
    return best;
}

// `launch(out)` starts one kernel that writes `n` floats at `out`; they come
// back once it has run.
template <class F>
std::vector<float> launch_fetch(size_t n, F&& launch) {
    DevBuf out(n * 4);
    launch(out.as<float>());
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    std::vector<float> h(n);
    HIP_CHECK(hipMemcpy(h.data(), out.p, n * 4, hipMemcpyDeviceToHost));
    return h;
}

inline int compute_units(int dev) {
    hipDeviceProp_t prop;
    HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    return prop.multiProcessorCount;
}

// A C-contiguous buffer of exactly `count` items of `itemsize` bytes.
inline const void* tile_buffer(const py::buffer_info& info, size_t itemsize,
                               size_t count, const char* what) {
    bool ok = (size_t)info.itemsize == itemsize && (size_t)info.size == count;
    py::ssize_t stride = info.itemsize;
    for (py::ssize_t d = info.ndim - 1; ok && d >= 0; d--) {
        if (info.shape[d] != 1 && info.strides[d] != stride) ok = false;
        stride *= info.shape[d];
    }
    require(ok, what);
    return info.ptr;
}

// A C-contiguous buffer of exactly `count` items of type T (by format code,
// so an int8 view is not taken for uint8 nor f32 for i32).
template <class T>
const T* typed_buffer(const py::buffer_info& info, size_t count, const char* what) {
    require(info.format == py::format_descriptor<T>::format(), what);
    return (const T*)tile_buffer(info, sizeof(T), count, what);
}

template <class T>
py::bytes as_bytes(const std::vector<T>& v) {
    return py::bytes(reinterpret_cast<const char*>(v.data()), v.size() * sizeof(T));
}

// Slabs of `slab` floats whose bits differ from slab 0. Every block of a
// tile launch computes the same thing, so a non-zero count is a sick CU.
inline uint64_t slab_mismatches(const std::vector<float>& d, size_t slab) {
    uint64_t bad = 0;
    for (size_t s = 1; s * slab < d.size(); s++)
        if (std::memcmp(d.data() + s * slab, d.data(), slab * sizeof(float)) != 0) bad++;
    return bad;
}

struct TileVerdict {
    bool ok;
    uint64_t bad_slabs;
};

// Slab 0 of `words` against the host's `ref`, every other slab against slab 0.
template <class T>
TileVerdict judge_tile(const std::vector<float>& words, const std::vector<T>& ref) {
    size_t slab = ref.size() * sizeof(T) / 4;
    return {std::memcmp(words.data(), ref.data(), slab * 4) == 0,
            slab_mismatches(words, slab)};
}

// The generator behind the probes' fixed tiles: 31 fresh bits per call.
inline uint32_t lcg_bits(uint64_t& s) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

inline int burn_blocks(int dev, int blocks, int per_cu) {
    return blocks > 0 ? blocks : compute_units(dev) * per_cu;
}

// Output elements whose bits differ from lane (i & 63) of block 0's wave 0.
// Every wave of the burn computes the same 64 values.
inline uint64_t burn_mismatches(const std::vector<float>& out) {
    uint64_t bad = 0;
    for (size_t i = WAVE; i < out.size(); i++)
        if (std::memcmp(&out[i], &out[i & (WAVE - 1)], 4) != 0) bad++;
    return bad;
}

// The burns share a launcher shape, launch(blocks, out, iters): `blocks`
// 256-thread workgroups that write blocks × 256 floats at `out`.

// What the raw burn entry points return: one launch, no warm-up.
template <class F>
py::dict raw_burn(F&& launch, int blocks, int iters) {
    std::vector<float> h = launch_fetch((size_t)blocks * 256, [&](float* out) {
        launch(blocks, out, iters);
    });
    py::dict d;
    d["lanes"] = py::bytes(reinterpret_cast<const char*>(h.data()), WAVE * 4);
    d["mismatches"] = burn_mismatches(h);
    d["blocks"] = blocks;
    return d;
}

struct TimedBurn {
    double tflops;
    float ms;
    uint64_t mismatches;
};

// What the probes run: a warm-up launch of 64 iterations, one timed launch of
// `iters` on the same buffer, and the check that all its waves agree bit for
// bit. `flops` is per block and iteration.
template <class F>
TimedBurn timed_burn(F&& launch, int blocks, int iters, double flops) {
    std::vector<float> h((size_t)blocks * 256);
    DevBuf out_buf(h.size() * 4);
    float* out = out_buf.as<float>();
    launch(blocks, out, 64);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipDeviceSynchronize());
    float ms = timed_ms([&] { launch(blocks, out, iters); });
    HIP_CHECK(hipMemcpy(h.data(), out, h.size() * 4, hipMemcpyDeviceToHost));
    return {(double)blocks * flops * iters / (ms * 1e9), ms, burn_mismatches(h)};
}

}  // namespace
