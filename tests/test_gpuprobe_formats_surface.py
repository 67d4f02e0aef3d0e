"""_gpuprobe_formats' Python-visible surface: the public names and each entry
point's signature with its defaults, as pybind11 renders them on the first
line of __doc__. Needs no GPU."""
import pytest

from kata_xpu_device_plugin_amd import _gpuprobe_formats as gf

INT = "typing.SupportsInt | typing.SupportsIndex"
BUF = "typing_extensions.Buffer"

SIGNATURES = {
    "mfma_f64_tile_run":
        f"mfma_f64_tile_run(dev: {INT}, A: {BUF}, B: {BUF}, C: object = None, "
        f"blocks: {INT} = 1) -> bytes",
    "mfma_f16_tile_run":
        f"mfma_f16_tile_run(dev: {INT}, A_bits: {BUF}, B_bits: {BUF}, "
        f"blocks: {INT} = 1) -> bytes",
    "mfma_i8_tile_run":
        f"mfma_i8_tile_run(dev: {INT}, A: {BUF}, B: {BUF}, C: object = None, "
        f"blocks: {INT} = 1) -> bytes",
    "smfmac_f16_tile_run":
        f"smfmac_f16_tile_run(dev: {INT}, A_bits: {BUF}, A_idx: {BUF}, B_bits: {BUF}, "
        f"blocks: {INT} = 1) -> bytes",
    "mfma_f64_burn_run":
        f"mfma_f64_burn_run(dev: {INT} = 0, iters: {INT} = 64, blocks: {INT} = 0) -> dict",
    "mfma_i8_burn_run":
        f"mfma_i8_burn_run(dev: {INT} = 0, iters: {INT} = 64, blocks: {INT} = 0) -> dict",
    "mfma_probe_formats":
        f"mfma_probe_formats(dev: {INT} = 0, burn_iters: {INT} = 20000) -> dict",
}


def test_public_names():
    assert {n for n in dir(gf) if not n.startswith("_")} == set(SIGNATURES)


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_signature(name):
    assert getattr(gf, name).__doc__.splitlines()[0] == SIGNATURES[name]


def test_the_first_extension_is_untouched():
    """The new entry points live here, not in _gpuprobe."""
    gp = pytest.importorskip("kata_xpu_device_plugin_amd._gpuprobe")
    assert not set(SIGNATURES) & set(dir(gp))
