"""_gpuprobe's Python-visible surface: the public names and each entry point's
signature with its defaults, as pybind11 renders them on the first line of
__doc__. Needs no GPU."""
import pytest

gp = pytest.importorskip("kata_xpu_device_plugin_amd._gpuprobe")

INT = "typing.SupportsInt | typing.SupportsIndex"
BUF = "typing_extensions.Buffer"

SIGNATURES = {
    "device_count": "device_count() -> int",
    "device_info": f"device_info(dev: {INT} = 0) -> dict",
    "hbm_bandwidth_probe":
        f"hbm_bandwidth_probe(dev: {INT} = 0, bytes: {INT} = 2147483648, "
        f"iters: {INT} = 5) -> dict",
    "hbm_copy_check": f"hbm_copy_check(dev: {INT} = 0, bytes: {INT} = 268435456) -> dict",
    "hbm_latency_probe":
        f"hbm_latency_probe(dev: {INT} = 0, bytes: {INT} = 1073741824, "
        f"steps: {INT} = 2000000) -> dict",
    "lds_bandwidth_probe": f"lds_bandwidth_probe(dev: {INT} = 0, iters: {INT} = 100000) -> dict",
    "lds_read_burn_run":
        f"lds_read_burn_run(dev: {INT} = 0, iters: {INT} = 256, blocks: {INT} = 0) -> bytes",
    "memtest":
        f"memtest(dev: {INT} = 0, bytes: {INT} = 2147483648, "
        f"corrupt_offsets: collections.abc.Sequence[{INT}] = [], "
        f"corrupt_xor: {INT} = 1) -> dict",
    "mfma_bf16_burn_run":
        f"mfma_bf16_burn_run(dev: {INT} = 0, iters: {INT} = 64, blocks: {INT} = 0) -> dict",
    "mfma_bf16_tile_run":
        f"mfma_bf16_tile_run(dev: {INT}, A_bits: {BUF}, B_bits: {BUF}, "
        f"blocks: {INT} = 1) -> bytes",
    "mfma_f32_tile_run":
        f"mfma_f32_tile_run(dev: {INT}, A: {BUF}, B: {BUF}, C: object = None, "
        f"blocks: {INT} = 1) -> bytes",
    "mfma_fp8_tile_run":
        f"mfma_fp8_tile_run(dev: {INT}, A_codes: {BUF}, B_codes: {BUF}, a_fmt: str, "
        f"b_fmt: str, blocks: {INT} = 1) -> bytes",
    "mfma_mx_burn_run":
        f"mfma_mx_burn_run(dev: {INT}, fmt: str, iters: {INT} = 64, blocks: {INT} = 0) -> dict",
    "mfma_mx_tile_run":
        f"mfma_mx_tile_run(dev: {INT}, A_codes: {BUF}, B_codes: {BUF}, A_scales: {BUF}, "
        f"B_scales: {BUF}, a_fmt: str, b_fmt: str, blocks: {INT} = 1) -> bytes",
    "mfma_probe_bf16": f"mfma_probe_bf16(dev: {INT} = 0, burn_iters: {INT} = 20000) -> dict",
    "mfma_probe_f32": f"mfma_probe_f32(dev: {INT} = 0) -> dict",
    "mfma_probe_lowp": f"mfma_probe_lowp(dev: {INT} = 0, burn_iters: {INT} = 20000) -> dict",
    "pcie_bandwidth_probe":
        f"pcie_bandwidth_probe(dev: {INT} = 0, bytes: {INT} = 268435456, "
        f"iters: {INT} = 5) -> dict",
    "unit_sweep_probe":
        f"unit_sweep_probe(dev: {INT} = 0, low_precision: bool = False, "
        f"reps: {INT} = 2) -> dict",
    "unit_sweep_run":
        f"unit_sweep_run(dev: {INT}, kinds: collections.abc.Sequence[str], reps: {INT}, "
        f"blocks: {INT} = 0, poison: object = None, threads: {INT} = 256) -> dict",
}


def test_public_names():
    names = {n for n in dir(gp) if not n.startswith("_")}
    assert names == set(SIGNATURES) | {"UNIT_SWEEP_DEFAULT_REPS"}
    assert gp.UNIT_SWEEP_DEFAULT_REPS == 2


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature(name):
    assert getattr(gp, name).__doc__.splitlines()[0] == SIGNATURES[name]
