"""GPU burn-in / validation built on the _gpuprobe HIP extension.

The reference has no vendor-library health at all (no
NVML; fsnotify only, generic_device_plugin.go:389-457) — these probes are
the MI355X-native additive capability SURVEY.md §2.2 calls for.

Use cases for a passthrough device plugin:
* pre-flight: before GPUs are vfio-bound (while still on amdgpu), verify
  each device's HBM bandwidth, matrix cores and memory integrity, and
  write the topology hint file — one command:
  ``python -m kata_xpu_device_plugin_amd.tools.burnin``;
* post-RAS validation after a device is returned from a VM.

On a GPU node the HIP extension is REQUIRED — a missing extension raises
instead of silently passing (the probes are the product here; a fallback
that probes nothing would report healthy hardware it never touched).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

from ..utils.log import get_logger

log = get_logger(__name__)

# Healthy-MI355X floors (MI355X_MICROARCH.md: HBM ≈6.3 TB/s achievable of
# 8 TB/s peak; bf16 MFMA ~2.5 PF dense chip-wide). Probes run alongside
# other tenants, so floors are deliberately conservative.
HBM_GBPS_FLOOR_MI355X = 4000.0
BF16_TFLOPS_FLOOR_MI355X = 1000.0
PCIE_GBPS_FLOOR = 20.0  # Gen5 x16 is ~63 GB/s; below 20 = degraded link
# Block-scaled MX burns (profiles/mfma_lowp.md): the smaller of 0.4× the
# guide's peak (~5 PF MX-fp8, ~10 PF MX-fp4) and 0.5× the measured median
# (4320 and 8237 TF).
MX_FP8_TFLOPS_FLOOR_MI355X = 2000.0
MX_FP4_TFLOPS_FLOOR_MI355X = 4000.0
# FP64 and INT8 burns (profiles/mfma_formats.md), by the same rule. No FP64
# matrix peak is on record here, so that floor is 0.5× the measured median
# (76.3 TF) alone; INT8 is 2× bf16 per clock (~5000 TOPS): the smaller of
# 0.4 × 5000 and 0.5 × the measured median (4487 TOPS).
F64_TFLOPS_FLOOR_MI355X = 38.0
I8_TOPS_FLOOR_MI355X = 2000.0


def _ext():
    try:
        from .. import _gpuprobe
    except ImportError as e:
        raise RuntimeError(
            "kata_xpu_device_plugin_amd._gpuprobe (HIP/gfx950) extension is "
            "not built; run `python -c 'from setup import build_hip; build_hip()'`"
        ) from e
    return _gpuprobe


def _ext_formats():
    """The FP64 / FP16 / INT8 / 2:4-sparse extension; loaded only for
    probe_device(matrix_formats=True)."""
    try:
        from .. import _gpuprobe_formats
    except ImportError as e:
        raise RuntimeError(
            "kata_xpu_device_plugin_amd._gpuprobe_formats (HIP/gfx950) extension "
            "is not built; run `python -c 'from setup import build_hip; build_hip()'`"
        ) from e
    return _gpuprobe_formats


@dataclass
class ProbeReport:
    device: int
    name: str = ""
    gcn_arch: str = ""
    compute_units: int = 0
    total_mem_gib: float = 0.0
    hbm_gbps: float = 0.0
    hbm_latency_ns: float = 0.0
    lds_tbps: float = 0.0
    pcie_h2d_gbps: float = 0.0
    pcie_d2h_gbps: float = 0.0
    bf16_tflops: float = 0.0
    mfma_f32_ok: bool = False
    mfma_bf16_ok: bool = False
    memtest_mismatches: int = -1
    # self-checks of what the probes computed (-1 = not run; 0 = healthy)
    hbm_copy_mismatches: int = -1
    hbm_chase_mismatches: int = -1
    lds_mismatches: int = -1
    mfma_f32_slab_mismatches: int = -1
    mfma_bf16_slab_mismatches: int = -1
    bf16_burn_mismatches: int = -1
    # low-precision matrix-core probes (probe_device(low_precision=True))
    mfma_fp8_ok: bool = False
    mfma_mx_fp8_ok: bool = False
    mfma_mx_fp4_ok: bool = False
    mx_fp8_tflops: float = 0.0
    mx_fp4_tflops: float = 0.0
    mfma_fp8_slab_mismatches: int = -1
    mfma_mx_fp8_slab_mismatches: int = -1
    mfma_mx_fp4_slab_mismatches: int = -1
    mx_fp8_burn_mismatches: int = -1
    mx_fp4_burn_mismatches: int = -1
    # FP64 / FP16 / INT8 / 2:4-sparse matrix-core probes
    # (probe_device(matrix_formats=True))
    mfma_f64_ok: bool = False
    mfma_f16_ok: bool = False
    mfma_i8_ok: bool = False
    mfma_sparse_f16_ok: bool = False
    mfma_f64_slab_mismatches: int = -1
    mfma_f16_slab_mismatches: int = -1
    mfma_i8_slab_mismatches: int = -1
    mfma_sparse_f16_slab_mismatches: int = -1
    f64_tflops: float = 0.0
    i8_tops: float = 0.0
    f64_burn_mismatches: int = -1
    i8_burn_mismatches: int = -1
    # placement-recording unit sweep (probe_device(unit_sweep=True))
    unit_sweep_ran: bool = False
    sweep_cus_seen: int = -1
    sweep_simds_seen: int = -1
    sweep_simds_missing: int = -1
    sweep_launches: int = 0
    sweep_ms: float = 0.0
    sweep_exclusive: bool = False
    faulty_units: List[Dict] = field(default_factory=list)
    passed: bool = False
    failures: List[str] = field(default_factory=list)

    def as_dict(self) -> Dict:
        return dict(self.__dict__)


def probe_device(
    dev: int = 0,
    bandwidth_bytes: int = 1 << 31,
    memtest_bytes: int = 1 << 31,
    burn_iters: int = 20000,
    hbm_floor_gbps: Optional[float] = None,
    tflops_floor: Optional[float] = None,
    low_precision: bool = False,
    fp8_tflops_floor: Optional[float] = None,
    fp4_tflops_floor: Optional[float] = None,
    unit_sweep: bool = False,
    matrix_formats: bool = False,
    f64_tflops_floor: Optional[float] = None,
    i8_tops_floor: Optional[float] = None,
) -> ProbeReport:
    """Run the full probe suite on one GPU; raises only on infrastructure
    errors — a sick GPU yields passed=False with reasons.

    `low_precision=True` adds the FP8 and block-scaled MX (FP8/FP4)
    matrix-core probes; they exist on gfx950 only.

    `unit_sweep=True` adds the placement-recording sweep: the exact tiles
    through every SIMD of every CU, failures named by XCD / SE / CU / SIMD,
    and incomplete coverage reported as a failure.

    `matrix_formats=True` adds the FP64, FP16, INT8 and 2:4-sparse
    matrix-core probes of the _gpuprobe_formats extension (gfx950 only)."""
    g = _ext()
    rep = ProbeReport(device=dev)
    info = g.device_info(dev)
    rep.name = info["name"]
    rep.gcn_arch = info["gcn_arch"]
    rep.compute_units = info["compute_units"]
    rep.total_mem_gib = info["total_mem_bytes"] / (1 << 30)

    is_mi355x = "gfx950" in rep.gcn_arch
    if hbm_floor_gbps is None:
        hbm_floor_gbps = HBM_GBPS_FLOOR_MI355X if is_mi355x else 100.0
    if tflops_floor is None:
        tflops_floor = BF16_TFLOPS_FLOOR_MI355X if is_mi355x else 10.0

    bw = g.hbm_bandwidth_probe(dev, bandwidth_bytes, 5)
    rep.hbm_gbps = bw["gbps"]
    if rep.hbm_gbps < hbm_floor_gbps:
        rep.failures.append(
            f"HBM bandwidth {rep.hbm_gbps:.0f} GB/s < floor {hbm_floor_gbps:.0f}"
        )

    rep.hbm_copy_mismatches = int(bw["copy_mismatches"])
    if rep.hbm_copy_mismatches:
        rep.failures.append(
            f"HBM copy: {rep.hbm_copy_mismatches} words of dst differ from src")

    lds = g.lds_bandwidth_probe(dev, max(2000, burn_iters))
    rep.lds_tbps = lds["tbps"]
    if is_mi355x and rep.lds_tbps < 80.0:
        rep.failures.append(
            f"LDS bandwidth {rep.lds_tbps:.0f} TB/s < floor 80 (b128 spec ≈150)")

    rep.lds_mismatches = int(lds["mismatches"])
    if rep.lds_mismatches:
        rep.failures.append(
            f"LDS read: {rep.lds_mismatches} lanes summed the wrong slots")

    lat = g.hbm_latency_probe(dev, min(bandwidth_bytes, 1 << 30), 500000)
    rep.hbm_latency_ns = lat["latency_ns"]
    if rep.hbm_latency_ns > 1500.0:
        rep.failures.append(
            f"HBM latency {rep.hbm_latency_ns:.0f} ns > 1500 (healthy ≈350)")

    rep.hbm_chase_mismatches = int(lat["final_index"] != lat["expected_index"])
    if rep.hbm_chase_mismatches:
        rep.failures.append(
            f"HBM pointer chase ended at {lat['final_index']}, "
            f"host walk at {lat['expected_index']}")

    pcie = g.pcie_bandwidth_probe(dev, min(bandwidth_bytes, 256 << 20), 5)
    rep.pcie_h2d_gbps = pcie["h2d_gbps"]
    rep.pcie_d2h_gbps = pcie["d2h_gbps"]
    for direction, v in (("H2D", rep.pcie_h2d_gbps), ("D2H", rep.pcie_d2h_gbps)):
        if v < PCIE_GBPS_FLOOR:
            rep.failures.append(
                f"PCIe {direction} {v:.1f} GB/s < floor {PCIE_GBPS_FLOOR:.0f} "
                "(degraded host link)"
            )

    f32 = g.mfma_probe_f32(dev)
    rep.mfma_f32_ok = bool(f32["ok"])
    if not rep.mfma_f32_ok:
        rep.failures.append(f"f32 MFMA mismatch (max_abs_err={f32['max_abs_err']})")

    rep.mfma_f32_slab_mismatches = int(f32["slab_mismatches"])
    if rep.mfma_f32_slab_mismatches:
        rep.failures.append(
            f"f32 MFMA: {rep.mfma_f32_slab_mismatches} blocks differ from block 0")

    bf16 = g.mfma_probe_bf16(dev, burn_iters)
    rep.mfma_bf16_ok = bool(bf16["ok"])
    rep.bf16_tflops = bf16["tflops"]
    if not rep.mfma_bf16_ok:
        rep.failures.append(f"bf16 MFMA mismatch (max_rel_err={bf16['max_rel_err']})")
    if rep.bf16_tflops < tflops_floor:
        rep.failures.append(
            f"bf16 MFMA {rep.bf16_tflops:.0f} TFLOP/s < floor {tflops_floor:.0f}"
        )

    rep.mfma_bf16_slab_mismatches = int(bf16["slab_mismatches"])
    if rep.mfma_bf16_slab_mismatches:
        rep.failures.append(
            f"bf16 MFMA: {rep.mfma_bf16_slab_mismatches} blocks differ from block 0")
    rep.bf16_burn_mismatches = int(bf16["burn_mismatches"])
    if rep.bf16_burn_mismatches:
        rep.failures.append(
            f"bf16 MFMA burn: {rep.bf16_burn_mismatches} lanes differ from wave 0")

    if low_precision:
        _probe_low_precision(g, rep, dev, burn_iters, is_mi355x,
                             fp8_tflops_floor, fp4_tflops_floor)

    if unit_sweep:
        _probe_unit_sweep(g, rep, dev, low_precision and is_mi355x)

    if matrix_formats:
        _probe_matrix_formats(rep, dev, burn_iters, is_mi355x,
                              f64_tflops_floor, i8_tops_floor)

    mt = g.memtest(dev, memtest_bytes)
    rep.memtest_mismatches = int(mt["mismatches"])
    if rep.memtest_mismatches:
        rep.failures.append(f"memtest: {rep.memtest_mismatches} mismatching words")

    rep.passed = not rep.failures
    log.info(
        "probe dev%d %s (%s, %d CUs, %.0f GiB): HBM %.0f GB/s @%.0f ns, "
        "LDS %.0f TB/s, PCIe %.0f/%.0f GB/s, bf16 %.0f TF — %s",
        dev, rep.name, rep.gcn_arch, rep.compute_units, rep.total_mem_gib,
        rep.hbm_gbps, rep.hbm_latency_ns, rep.lds_tbps,
        rep.pcie_h2d_gbps, rep.pcie_d2h_gbps, rep.bf16_tflops,
        "PASS" if rep.passed else rep.failures,
    )
    return rep


def _probe_low_precision(g, rep: ProbeReport, dev: int, burn_iters: int,
                         is_mi355x: bool, fp8_tflops_floor: Optional[float],
                         fp4_tflops_floor: Optional[float]) -> None:
    """FP8 / MX-fp8 / MX-fp4 tiles and MX burns; one failure per failed check."""
    if not is_mi355x:
        # v_mfma_*_fp8 (OCP) and v_mfma_scale_* do not exist elsewhere
        rep.failures.append(
            f"low-precision MFMA probes skipped: {rep.gcn_arch or 'unknown arch'} "
            "is not gfx950")
        return
    if fp8_tflops_floor is None:
        fp8_tflops_floor = MX_FP8_TFLOPS_FLOOR_MI355X
    if fp4_tflops_floor is None:
        fp4_tflops_floor = MX_FP4_TFLOPS_FLOOR_MI355X
    lp = g.mfma_probe_lowp(dev, burn_iters)
    for label, key in (("fp8", "fp8"), ("MX-fp8", "mx_fp8"), ("MX-fp4", "mx_fp4")):
        ok = bool(lp[f"{key}_ok"])
        slabs = int(lp[f"{key}_slab_mismatches"])
        setattr(rep, f"mfma_{key}_ok", ok)
        setattr(rep, f"mfma_{key}_slab_mismatches", slabs)
        if not ok:
            rep.failures.append(
                f"{label} MFMA mismatch (exact tile differs from the host product)")
        if slabs:
            rep.failures.append(f"{label} MFMA: {slabs} blocks differ from block 0")
    for label, key, floor in (("MX-fp8", "mx_fp8", fp8_tflops_floor),
                              ("MX-fp4", "mx_fp4", fp4_tflops_floor)):
        tflops = float(lp[f"{key}_tflops"])
        burn = int(lp[f"{key}_burn_mismatches"])
        setattr(rep, f"{key}_tflops", tflops)
        setattr(rep, f"{key}_burn_mismatches", burn)
        if burn:
            rep.failures.append(f"{label} MFMA burn: {burn} lanes differ from wave 0")
        if tflops < floor:
            rep.failures.append(
                f"{label} MFMA {tflops:.0f} TFLOP/s < floor {floor:.0f}")


def _probe_matrix_formats(rep: ProbeReport, dev: int, burn_iters: int,
                          is_mi355x: bool, f64_tflops_floor: Optional[float],
                          i8_tops_floor: Optional[float]) -> None:
    """FP64 / FP16 / INT8 / 2:4-sparse tiles and the FP64 and INT8 burns; one
    failure per failed check. The extension is loaded only here."""
    if not is_mi355x:
        # the kernels are built for gfx950; the K=64 i8 and sparse forms and
        # the 32x32x16 f16 form do not exist elsewhere
        rep.failures.append(
            f"matrix-format MFMA probes skipped: {rep.gcn_arch or 'unknown arch'} "
            "is not gfx950")
        return
    if f64_tflops_floor is None:
        f64_tflops_floor = F64_TFLOPS_FLOOR_MI355X
    if i8_tops_floor is None:
        i8_tops_floor = I8_TOPS_FLOOR_MI355X
    mf = _ext_formats().mfma_probe_formats(dev, burn_iters)
    for label, key in (("f64", "f64"), ("f16", "f16"), ("i8", "i8"),
                       ("2:4-sparse f16", "sparse_f16")):
        ok = bool(mf[f"{key}_ok"])
        slabs = int(mf[f"{key}_slab_mismatches"])
        setattr(rep, f"mfma_{key}_ok", ok)
        setattr(rep, f"mfma_{key}_slab_mismatches", slabs)
        if not ok:
            rep.failures.append(
                f"{label} MFMA mismatch (exact tile differs from the host product)")
        if slabs:
            rep.failures.append(f"{label} MFMA: {slabs} blocks differ from block 0")
    for label, key, rate, unit, floor in (
            ("f64", "f64", "f64_tflops", "TFLOP/s", f64_tflops_floor),
            ("i8", "i8", "i8_tops", "TOP/s", i8_tops_floor)):
        value = float(mf[rate])
        burn = int(mf[f"{key}_burn_mismatches"])
        setattr(rep, rate, value)
        setattr(rep, f"{key}_burn_mismatches", burn)
        if burn:
            rep.failures.append(f"{label} MFMA burn: {burn} lanes differ from wave 0")
        if value < floor:
            rep.failures.append(
                f"{label} MFMA {value:.0f} {unit} < floor {floor:.0f}")


def _probe_unit_sweep(g, rep: ProbeReport, dev: int, low_precision: bool) -> None:
    """The unit sweep: one failure line per faulty unit and kind, one for
    incomplete coverage, one for a suspect id layout, one per kind whose
    golden tile could not be trusted."""
    from . import placement

    sw = g.unit_sweep_probe(dev, low_precision)
    summary = placement.summarise(sw["records"], rep.compute_units,
                                  int(sw["waves_per_block"]))
    rep.unit_sweep_ran = True
    rep.sweep_cus_seen = int(summary["cus_seen"])
    rep.sweep_simds_seen = int(summary["simds_seen"])
    rep.sweep_simds_missing = int(summary["missing"])
    rep.sweep_launches = int(sw["launches"])
    rep.sweep_ms = float(sw["sweep_ms"])
    rep.sweep_exclusive = bool(sw["exclusive"])
    reps = int(sw["reps"])
    for kind, ok in sw["golden_ok"].items():
        if not ok:
            rep.failures.append(
                f"unit sweep: no trusted golden {placement.KIND_LABEL[kind]}, "
                "kind not swept")
    for f in summary["faulty_units"]:
        unit, kind = f["unit"], f["kind"]
        name = placement.format_unit(unit)
        rep.faulty_units.append({
            "unit": name, "kind": kind, "xcd": unit.xcd, "se": unit.se,
            "sh": unit.sh, "cu": unit.cu, "simd": unit.simd,
            "mismatches": f["mismatches"], "waves": f["waves"],
            "hw_id": f["hw_id"], "xcc_id": f["xcc_id"],
        })
        if kind == "lds":
            detail = f"{f['mismatches']} wrong words in {f['waves']} waves' read-back"
        else:
            detail = (f"{f['mismatches']} wrong elements in {f['waves']} waves "
                      f"x {reps} repetitions")
        rep.failures.append(
            f"unit sweep: {placement.KIND_LABEL[kind]} wrong on {name} ({detail})")
    if rep.sweep_simds_missing:
        line = (f"unit sweep: {rep.sweep_simds_missing} of "
                f"{summary['simds_expected']} SIMDs never ran it")
        if summary["partial_cus"]:
            line += " (CUs seen in part: " + ", ".join(
                f"{c['unit']} SIMDs {c['simds_seen']}"
                for c in summary["partial_cus"][:8]) + ")"
        rep.failures.append(line)
    if summary["layout_suspect"]:
        rep.failures.append(
            f"unit sweep: hardware ids do not fit the assumed layout "
            f"({rep.sweep_cus_seen} CU keys on {rep.compute_units} CUs, or one "
            "workgroup on two CUs); unit names are not to be trusted")


def _probe_as_dict(dev: int, kw: Dict) -> Dict:
    """Top-level helper for spawn-based multiprocessing."""
    return probe_device(dev, **kw).as_dict()


def probe_all(parallel: bool = False, **kw) -> List[ProbeReport]:
    """Probe every visible GPU; `parallel=True` runs one spawned process
    per GPU (own HIP context) — cuts an 8-GPU pre-flight ~8×. HIP state
    must not leak across fork, hence the spawn context."""
    g = _ext()
    n = g.device_count()
    if not parallel or n <= 1:
        return [probe_device(i, **kw) for i in range(n)]
    import concurrent.futures as cf
    import multiprocessing as mp

    reports: List[ProbeReport] = []
    with cf.ProcessPoolExecutor(
        max_workers=n, mp_context=mp.get_context("spawn")
    ) as pool:
        for d in pool.map(_probe_as_dict, range(n), [kw] * n):
            rep = ProbeReport(device=d["device"])
            rep.__dict__.update(d)
            reports.append(rep)
    return reports
