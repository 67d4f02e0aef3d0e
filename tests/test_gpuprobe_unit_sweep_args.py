"""Argument validation of the unit-sweep entry points: every bad argument is a
ValueError raised before the first HIP call, so these run without a GPU."""
import pytest

gp = pytest.importorskip("kata_xpu_device_plugin_amd._gpuprobe")

ALL = ["f32", "bf16", "fp8", "mx_fp8", "mx_fp4", "lds"]


def test_negative_device():
    with pytest.raises(ValueError, match="dev"):
        gp.unit_sweep_run(-1, ALL, 8)
    with pytest.raises(ValueError, match="dev"):
        gp.unit_sweep_probe(-1)


@pytest.mark.parametrize("reps", [0, -1, (1 << 20) + 1])
def test_reps_range(reps):
    with pytest.raises(ValueError, match="reps"):
        gp.unit_sweep_run(0, ALL, reps)
    with pytest.raises(ValueError, match="reps"):
        gp.unit_sweep_probe(0, False, reps)
    with pytest.raises(ValueError, match="reps"):
        gp.unit_sweep_probe(0, low_precision=True, reps=reps)


@pytest.mark.parametrize("blocks", [-1, 4097, 1 << 20])
def test_blocks_range(blocks):
    with pytest.raises(ValueError, match="blocks"):
        gp.unit_sweep_run(0, ALL, 8, blocks)


@pytest.mark.parametrize("kinds", [[], ["f64"], ["f32", "LDS"], ["f32", ""]])
def test_kinds_must_be_a_non_empty_subset(kinds):
    with pytest.raises(ValueError, match="kinds"):
        gp.unit_sweep_run(0, kinds, 8)


@pytest.mark.parametrize("threads", [0, 64, 128, 384, 2048])
def test_threads_choice(threads):
    with pytest.raises(ValueError, match="threads"):
        gp.unit_sweep_run(0, ALL, 8, threads=threads)


@pytest.mark.parametrize("poison", [
    (16, 0, 0, "bf16", 1),            # xcc_id
    (-1, 0, 0, "bf16", 1),
    (0, 256, 0, "bf16", 1),           # cu_key
    (0, -1, 0, "bf16", 1),
    (0, 0, 4, "bf16", 1),             # simd_id
    (0, 0, -1, "bf16", 1),
    (0, 0, 0, "bf17", 1),             # kind
    (0, 0, 0, "bf16", 0),             # xor_bits
    (0, 0, 0, "bf16", 1 << 32),
    (0, 0, 0, "bf16", -1),
    (0, 0, 0, "bf16"),                # shape and types
    (0, 0, 0, "bf16", 1, 2),
    (0, 0, 0, 3, 1),
    ("0", 0, 0, "bf16", 1),
    7,
])
def test_poison_fields(poison):
    with pytest.raises(ValueError, match="poison"):
        gp.unit_sweep_run(0, ALL, 8, poison=poison)


def test_poison_kind_must_be_selected():
    with pytest.raises(ValueError, match="poison kind"):
        gp.unit_sweep_run(0, ["f32", "lds"], 8, poison=(0, 0, 0, "bf16", 1))


def test_default_reps_is_exported_and_in_range():
    assert 1 <= gp.UNIT_SWEEP_DEFAULT_REPS <= 1 << 20
