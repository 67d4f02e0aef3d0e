"""Where the unit sweep's waves ran: decode the hardware ids a wave read in
the kernel, and summarise a launch's records into coverage and faulty units.

Pure Python, no GPU needed. A record is eight uint32 in the order the kernel
writes them (probes/xpu_probe.hip, unit_sweep):

    hw_id, xcc_id, bad_f32, bad_bf16, bad_fp8, bad_mx_fp8, bad_mx_fp4, bad_lds

The bit layout of HW_ID is the gfx9 one from AMD's CDNA3 ISA guide and
LLVM's SIDefines.h. What an MI355X was seen to report is in
profiles/unit_sweep.md. Because the layout is taken from documents, the
summary treats (xcd, HW_ID bits 15:8) as an opaque CU key, never assumes the
keys are dense (harvested parts skip CU ids), keeps the raw words, and flags
records that no correct decode could produce (`layout_suspect`).
"""
from __future__ import annotations

import struct
from typing import Dict, Iterable, List, NamedTuple, Sequence, Tuple, Union

RECORD_WORDS = 8
# record word index of each kind's mismatch counter
KIND_WORD = {"f32": 2, "bf16": 3, "fp8": 4, "mx_fp8": 5, "mx_fp4": 6, "lds": 7}
KINDS = tuple(KIND_WORD)
BASE_KINDS = ("f32", "bf16", "lds")
LOW_PRECISION_KINDS = ("fp8", "mx_fp8", "mx_fp4")
KIND_LABEL = {"f32": "f32 tile", "bf16": "bf16 tile", "fp8": "fp8 tile",
              "mx_fp8": "MX-fp8 tile", "mx_fp4": "MX-fp4 tile", "lds": "LDS"}
SIMDS_PER_CU = 4


class Unit(NamedTuple):
    """One place on the die. `simd` and `wave_slot` are -1 where they do not
    apply (an LDS fault belongs to the CU; a faulty unit is not one slot)."""
    xcd: int
    se: int
    sh: int
    cu: int
    simd: int
    wave_slot: int


def decode(hw_id: int, xcc_id: int) -> Unit:
    """HW_ID: WAVE_ID[3:0] SIMD_ID[5:4] CU_ID[11:8] SH_ID[12] SE_ID[15:13];
    XCC_ID[3:0] of the other register. Higher bits (TG / VM / QUEUE / STATE /
    ME) are ignored."""
    return Unit(
        xcd=xcc_id & 0xF,
        se=(hw_id >> 13) & 0x7,
        sh=(hw_id >> 12) & 0x1,
        cu=(hw_id >> 8) & 0xF,
        simd=(hw_id >> 4) & 0x3,
        wave_slot=hw_id & 0xF,
    )


def cu_key(hw_id: int, xcc_id: int) -> Tuple[int, int]:
    """(xcd, HW_ID bits 15:8): names a CU without trusting the SE/SH/CU split."""
    return (xcc_id & 0xF, (hw_id >> 8) & 0xFF)


def format_unit(unit: Unit) -> str:
    """"XCD 3 SE 1 CU 7 SIMD 2"; the SIMD is left out where it does not apply
    (LDS) and the SH is named only when it is not 0."""
    parts = [f"XCD {unit.xcd}", f"SE {unit.se}"]
    if unit.sh:
        parts.append(f"SH {unit.sh}")
    parts.append(f"CU {unit.cu}")
    if unit.simd >= 0:
        parts.append(f"SIMD {unit.simd}")
    return " ".join(parts)


Records = Union[bytes, bytearray, memoryview, Iterable[Sequence[int]]]


def unpack(records: Records) -> List[Tuple[int, ...]]:
    """Raw little-endian bytes (or rows of eight ints) → list of 8-tuples."""
    if isinstance(records, (bytes, bytearray, memoryview)):
        raw = bytes(records)
        if len(raw) % (4 * RECORD_WORDS):
            raise ValueError("records: length is not a multiple of 32 bytes")
        return list(struct.iter_unpack("<8I", raw))
    rows = [tuple(int(w) for w in r) for r in records]
    for r in rows:
        if len(r) != RECORD_WORDS:
            raise ValueError("records: a record is eight uint32")
    return rows


def summarise(records: Records, compute_units: int, waves_per_block: int) -> Dict:
    """Coverage and faults of one or several merged launches.

    Records of merged launches may name the same SIMD many times; it counts
    once. Consecutive groups of `waves_per_block` records are one workgroup.
    """
    if waves_per_block < 1:
        raise ValueError("waves_per_block must be >= 1")
    rows = unpack(records)
    simds_by_cu: Dict[Tuple[int, int], set] = {}
    raw_by_cu: Dict[Tuple[int, int], Tuple[int, int]] = {}
    # (unit, kind) → [mismatches, waves, hw_id and xcc_id of the first wave]
    faults: Dict[Tuple[Unit, str], List[int]] = {}
    block_spans_cus = False
    for i, r in enumerate(rows):
        hw_id, xcc_id = r[0], r[1]
        key = cu_key(hw_id, xcc_id)
        u = decode(hw_id, xcc_id)
        simds_by_cu.setdefault(key, set()).add(u.simd)
        raw_by_cu.setdefault(key, (hw_id, xcc_id))
        if i % waves_per_block and key != cu_key(rows[i - 1][0], rows[i - 1][1]):
            block_spans_cus = True
        for kind, w in KIND_WORD.items():
            if not r[w]:
                continue
            where = u._replace(wave_slot=-1, simd=-1 if kind == "lds" else u.simd)
            f = faults.setdefault((where, kind), [0, 0, hw_id, xcc_id])
            f[0] += r[w]
            f[1] += 1

    simds_expected = SIMDS_PER_CU * compute_units
    simds_seen = sum(len(s) for s in simds_by_cu.values())
    partial = []
    for key in sorted(simds_by_cu):
        if len(simds_by_cu[key]) < SIMDS_PER_CU:
            hw_id, xcc_id = raw_by_cu[key]
            partial.append({
                "xcd": key[0], "cu_key": key[1],
                "unit": format_unit(decode(hw_id, xcc_id)._replace(simd=-1, wave_slot=-1)),
                "simds_seen": sorted(simds_by_cu[key]),
            })
    faulty = [
        {"unit": where, "kind": kind, "mismatches": f[0], "waves": f[1],
         "hw_id": f[2], "xcc_id": f[3]}     # raw words of the first such wave
        for (where, kind), f in sorted(faults.items(),
                                       key=lambda kv: (kv[0][0], KINDS.index(kv[0][1])))
    ]
    return {
        "cus_seen": len(simds_by_cu),
        "simds_seen": simds_seen,
        "simds_expected": simds_expected,
        "xcds_seen": len({k[0] for k in simds_by_cu}),
        "missing": max(0, simds_expected - simds_seen),
        "partial_cus": partial,
        "faulty_units": faulty,
        # more CUs than the device has, or one workgroup on two CUs: only a
        # wrong decode can say that
        "layout_suspect": len(simds_by_cu) > compute_units or block_spans_cus,
    }
