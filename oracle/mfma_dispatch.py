"""Which int8 matrix-core ring kernel a launch reaches: the dispatch of ``ring_launch_multi`` / ``ring_launch_pairs``
(csrc/channelize_ring.hip) restated on the host, and the sweep of launches tests/test_gpu_mfma_exact.py runs so that
every instantiation is compared with the exact model (oracle/mfma_model.py) once.

The ABI's queries (``iqa_mfma_ring_mode`` / ``_lanes`` / ``_pairs``) see the slot form (contiguous or row-staged) and
whether pairs exist, not the SKIPK / HALF / 64-bit choice inside a form: ``abi_agrees`` checks what they can see, the
rest rests on this restatement (a kernel trace of the sweep lists the same instantiations, each as often as the sweep
names it).  Test infrastructure only: the package never imports it.
"""
from __future__ import annotations

RG_MAX_KS = 16
RG_ROWS_MAX_KS = 11
PAIR_KS = (9, 10, 11, 12, 13, 14, 16)  # lane pairs, int32 sums (not 15: registers)
PAIR64_KS = tuple(range(9, 15))


def ring_mode(fmt: str, d: int, k_first: int, k_count: int, acc64: bool) -> int:
    """``mfma_ring_mode``: 1 = contiguous slots, 2 = row-staged slots, 0 = none."""
    ks_all = -(-2 * d // 32)
    if fmt != "u8" and d >= 4 and d % 4 == 0 and ks_all <= (RG_MAX_KS - 1 if acc64 else RG_MAX_KS) and k_first == 0 \
            and k_count == ks_all:
        return 1
    if not acc64 and 1 <= k_count <= RG_ROWS_MAX_KS and k_first >= 0 and k_first + k_count <= ks_all:
        return 2
    return 0


def expected_kernel(entry: str, fmt: str, d: int, k_first: int, k_count: int, acc64: bool, skipk: bool) -> str:
    """The instantiation ``entry`` ("multi": iqa_channelize_mfma_multi, "pairs": iqa_channelize_mfma_pairs) dispatches
    to, as name<KS[, SKIPK]> (``...64``: 64-bit sums).  ``skipk``: the launch takes the q2*hi-skipping variant (multi:
    some lane is high-byte-only; pairs: every first lane is and no second lane is)."""
    mode = ring_mode(fmt, d, k_first, k_count, acc64)
    assert mode, "no ring kernel"
    ks = k_count
    sk = ", SKIPK" if skipk else ""
    if entry == "pairs":
        assert mode == 1 and ks in (PAIR64_KS if acc64 else PAIR_KS)
        return f"k_channelize_mfma_s16_ring_pairs{'64' if acc64 else ''}<{ks}{sk}>"
    if acc64:
        assert mode == 1
        return f"k_channelize_mfma_s16_ring_multi64<{ks}{sk}>"
    if mode == 2:
        if fmt == "u8":
            return f"k_channelize_mfma_u8_ring_rows_multi<{ks}>"
        return f"k_channelize_mfma_s16_ring_rows_multi<{ks}{sk}>"
    if skipk:
        return f"k_channelize_mfma_s16_ring_multi<{ks}, SKIPK>"
    rem = (2 * d) & 31  # values in the row's last k step
    if ks <= 8 and rem != 0 and rem <= 16:
        return f"k_channelize_mfma_s16_ring_multi_half<{ks}>"
    return f"k_channelize_mfma_s16_ring_multi<{ks}>"


def all_ring_instantiations() -> set:
    """Every kernel the two launchers can select (129)."""
    s = set()
    for ks in range(1, RG_MAX_KS + 1):
        s |= {f"k_channelize_mfma_s16_ring_multi<{ks}>", f"k_channelize_mfma_s16_ring_multi<{ks}, SKIPK>"}
    for ks in range(1, 9):
        s.add(f"k_channelize_mfma_s16_ring_multi_half<{ks}>")
    for ks in range(1, RG_MAX_KS):
        s |= {f"k_channelize_mfma_s16_ring_multi64<{ks}>", f"k_channelize_mfma_s16_ring_multi64<{ks}, SKIPK>"}
    for ks in range(1, RG_ROWS_MAX_KS + 1):
        s |= {f"k_channelize_mfma_s16_ring_rows_multi<{ks}>", f"k_channelize_mfma_s16_ring_rows_multi<{ks}, SKIPK>",
              f"k_channelize_mfma_u8_ring_rows_multi<{ks}>"}
    for ks in PAIR_KS:
        s |= {f"k_channelize_mfma_s16_ring_pairs<{ks}>", f"k_channelize_mfma_s16_ring_pairs<{ks}, SKIPK>"}
    for ks in PAIR64_KS:
        s |= {f"k_channelize_mfma_s16_ring_pairs64<{ks}>", f"k_channelize_mfma_s16_ring_pairs64<{ks}, SKIPK>"}
    return s


def sweep_cases() -> list:
    """(kind, KS, D) of the instantiation sweep: one launch per case, all k steps of a row in one pass."""
    cases = []
    for ks in range(1, 17):
        cases += [("multi", ks, 16 * ks), ("multi_skip", ks, 16 * ks)]
    for ks in (1, 3, 7, 13, 16):
        cases.append(("multi", ks, 16 * ks - 4))  # D = 12 mod 16: 24 values in the row's last k step, no half step
    for ks in range(1, 9):
        cases.append(("multi_half", ks, 16 * ks - (8 if ks % 2 else 12)))  # 16 or 8 values in the last k step
    for ks in range(1, 16):
        cases += [("multi64", ks, 16 * ks), ("multi64_skip", ks, 16 * ks)]
    for ks in range(1, 12):
        cases += [("rows", ks, 16 * ks - 3), ("rows_skip", ks, 16 * ks - 3), ("u8", ks, 16 * ks - 3)]  # odd D
    for ks in PAIR_KS:
        cases += [("pairs", ks, 16 * ks), ("pairs_skip", ks, 16 * ks)]
    for ks in PAIR64_KS:
        cases += [("pairs64", ks, 16 * ks), ("pairs64_skip", ks, 16 * ks)]
    return cases


def case_launch(kind: str, ks: int, d: int):
    """(entry, fmt, acc64, skipk) of a sweep case."""
    return ("pairs" if kind.startswith("pairs") else "multi", "u8" if kind == "u8" else "s16", "64" in kind,
            kind.endswith("skip"))


def sweep_kernel(kind: str, ks: int, d: int) -> str:
    entry, fmt, acc64, skipk = case_launch(kind, ks, d)
    return expected_kernel(entry, fmt, d, 0, ks, acc64, skipk)


def abi_agrees(lib, entry: str, fmt: str, d: int, k_first: int, k_count: int, acc64: bool, name: str) -> None:
    """The library's own queries agree with ``expected_kernel``'s slot form and pair availability for this launch."""
    code = {"s16": 0, "u8": 1}[fmt]
    acc32 = 0 if acc64 else 1
    mode = lib.iqa_mfma_ring_mode(code, d, k_first, k_count, acc32)
    lanes = lib.iqa_mfma_ring_lanes(code, d, k_first, k_count, acc32)
    assert mode == ring_mode(fmt, d, k_first, k_count, acc64) == (2 if "rows" in name else 1), (name, mode)
    assert lanes & 1, name
    if entry == "pairs":
        assert lanes & 2 and (acc64 or lib.iqa_mfma_ring_pairs(code, d, k_first, k_count) == 1), name
    elif fmt == "s16" and not acc64:
        assert bool(lanes & 2) == bool(lib.iqa_mfma_ring_pairs(code, d, k_first, k_count)), name
