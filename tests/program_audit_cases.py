"""Inputs the program audit's CPU and GPU tests share: the captured two-chip `rom` machine (tests/air_script.py opens the AIRs: a `fetcher`
with columns pc, f0..f(n-1) that sends its row with count one on global bus 1, and a `table` with the main column multiplicity and the
preprocessed columns key, w0..w(n-1) that receives its preprocessed row with count multiplicity: the reference's commented-out program bus
restated), its clean traces from a list of pcs, the tamperings, the edge traces, and the VM witnesses of the BasicMachine with their ROM
lengths and the tampered fib(25).  Everything is built in numpy, nothing is random."""
import ctypes

import numpy as np

import air_script
import valida_amd as va
from domain_audit_cases import Interaction, Vcol, VcolTerm

P = va.P
TWO32 = (1 << 32) % P
CPU, PROGRAM, BUS = 0, 1, 1
FETCH_HEIGHTS = (1, 2, 64, 128, 256, 512, 2048, 4096, 8192)
TABLE_HEIGHTS = (1, 2, 32, 32768, 65536)
PLANT_ROWS = (63, 64, 255, 256, 2047, 2048, 4097)
_machines = {}


def _vcol(terms, constant=0):
    arr = (VcolTerm * max(1, len(terms)))(*[VcolTerm(int(p), c, w) for p, c, w in terms])
    v = Vcol(arr, len(terms), constant)
    v._keep = arr
    return v


def rom_machine(n_fields=2):
    """The captured machine, one per field count."""
    if n_fields in _machines:
        return _machines[n_fields]
    L, u = va.lib(), ctypes.c_uint32
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0
    chips = [(air_script.Script("fetcher", 1 + n_fields, 0, []), True, [_vcol([(0, k, 1)]) for k in range(1 + n_fields)], _vcol([], 1)),
             (air_script.Script("table", 1, 1 + n_fields, []), False, [_vcol([(1, k, 1)]) for k in range(1 + n_fields)], _vcol([(0, 0, 1)]))]
    for script, is_send, fields, count in chips:
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(script.name.encode(), u(script.width), u(script.prep_width), ctypes.byref(air)) == 0
        air_script.capture(L, air, script)  # no constraints: the chips are their interactions
        arr = (Vcol * len(fields))(*fields)
        it = Interaction(arr, len(fields), count, 1, BUS, int(is_send))
        assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)
    _machines[n_fields] = va.Machine(m)
    return _machines[n_fields]


def rom_opts(n_fields=2):
    """fetch = and table = of the audit for the `rom` machine."""
    cols = list(range(1, 1 + n_fields))
    return dict(fetch=(0, 0, cols), table=(1, 0, cols, 0))


def words(T, n_fields=2):
    """The table's words: distinct rows, values below and near p."""
    i, j = np.arange(T, dtype=np.int64)[:, None], np.arange(n_fields, dtype=np.int64)[None, :]
    return (i * 2654435761 + j * 40503 + (i % 5 == 0) * (P - 3)) % P


def clean(pcs, T, n_fields=2):
    """(main traces, preprocessed) of a truthful witness that fetches `pcs` (all below T) from a table of T rows."""
    pcs = np.asarray(pcs, dtype=np.int64)
    W = words(T, n_fields)
    fetch = np.concatenate([pcs[:, None], W[pcs]], axis=1).astype(np.uint32)
    mult = (np.bincount(pcs, minlength=T) % P).astype(np.uint32)[:, None]
    prep = np.concatenate([np.arange(T, dtype=np.int64)[:, None], W], axis=1).astype(np.uint32)
    return [fetch, mult], [(1, prep)]


def loop_pcs(H, T):
    return np.arange(H, dtype=np.int64) % T


TAMPERINGS = ("operand", "wrapped", "pc_other_word", "pc_padding", "pc_p_minus_1", "multiplicity", "key")


def tamper(main, prep, kind, fetch_chip, pc_col, field_col, table_chip, mult_col, key_col, row=100, other_pc=None, padding_pc=31):
    """One of TAMPERINGS applied to copies of (main, prep)."""
    main, prep = [m.copy() for m in main], [(c, m.copy()) for c, m in prep]
    f, t, p = main[fetch_chip], main[table_chip], dict(prep)[table_chip]
    if kind == "operand":
        f[row, field_col] = (int(f[row, field_col]) + 7) % P
    elif kind == "wrapped":
        f[row, field_col] = (int(f[row, field_col]) + TWO32) % P
    elif kind == "pc_other_word":
        f[row, pc_col] = other_pc
    elif kind == "pc_padding":
        f[row, pc_col] = padding_pc
    elif kind == "pc_p_minus_1":
        f[row, pc_col] = P - 1
    elif kind == "multiplicity":
        t[3, mult_col] = (int(t[3, mult_col]) + 1) % P
    else:
        p[5, key_col] = 6
    return main, prep


def rom_tampered(kind, H=256, T=32):
    main, prep = clean(loop_pcs(H, T), T)
    return tamper(main, prep, kind, 0, 0, 1, 1, 0, 0, other_pc=(100 % T + 9) % T)


def skipping():
    """A five-word program whose always-taken branch skips words 2 and 3: 0, 1, 4, 4, .. in a table of 8 rows, rom_len 5."""
    return clean([0, 1, 4, 4, 4, 4, 4, 4], 8), 5


def planted(rows=PLANT_ROWS, H=8192, T=32):
    """A wrong operand at each of `rows`: a wave, a workgroup, a histogram run and one row past them."""
    main, prep = clean(loop_pcs(H, T), T)
    for r in rows:
        main[0][r, 2] = (int(main[0][r, 2]) + 1) % P
    return main, prep


def many(H=1024, T=1024, k=300):
    """k wrong instructions, k wrapped operands, k wrong keys and multiplicities, and alternating fetched and unfetched words (T / 2 ranges)."""
    main, prep = clean(2 * (np.arange(H, dtype=np.int64) % (T // 2)), T)
    for r in range(k):
        main[0][2 * r, 1] = (int(main[0][2 * r, 1]) + 5) % P
        main[0][2 * r + 1, 2] = (int(main[0][2 * r + 1, 2]) + TWO32) % P
        main[1][r, 0] = (int(main[1][r, 0]) + 1) % P
        prep[0][1][T - 1 - r, 0] = 0
    return main, prep


def edge_cases():
    """[(name, n_fields, (main, prep), rom_len)]: what the host, the emulated kernels and the device are held to."""
    out = []
    for H in FETCH_HEIGHTS:
        out.append(("fetch_height_%d" % H, 2, clean(loop_pcs(H, 23), 32), 23 if H >= 32 else 0))
    for T in TABLE_HEIGHTS:
        out.append(("table_height_%d" % T, 2, clean((np.arange(4096, dtype=np.int64) * 37) % T, T), 0))
    out.append(("one_pc", 2, clean(np.full(4096, 7), 32), 0))
    lanes = np.full(256, 7)
    lanes[[5, 64 + 63, 128]] = 9  # three waves with 63 lanes on one pc and one lane on another, one wave uniform
    out.append(("63_and_1", 2, clean(lanes, 32), 0))
    out.append(("two_bins", 2, clean(3 + 8 * (np.arange(2048) % 2), 32), 0))
    hot = np.array([0, 32767, 32768, 65535])[np.arange(8192) // 3 % 4]  # runs of three: uniform and mixed waves on the slice edges
    out.append(("slice_edges", 2, clean(hot, 65536), 0))
    for kind in TAMPERINGS:
        out.append(("tampered_" + kind, 2, rom_tampered(kind), 23 if kind == "pc_padding" else 0))
    out.append(("planted", 2, planted(), 0))
    out.append(("skipping", 2) + skipping())
    out.append(("one_field", 1, clean(loop_pcs(512, 32), 32, 1), 0))
    m8 = clean(loop_pcs(512, 32), 32, 8)
    m8[0][0][300, 8] = (int(m8[0][0][300, 8]) + 1) % P
    m8[0][0][301, 1] = (int(m8[0][0][301, 1]) + TWO32) % P
    out.append(("eight_fields", 8, m8, 0))
    return out


def big_bin(H=1 << 17):
    """A bin count above 2^16: every fetch on word 1 of a two-row table."""
    return clean(np.full(H, 1), 2)


def synthetic(H, T=256):
    """H fetches of a T-word table in a fixed pattern (runs, strides and a hot word), every 997th row a wrong operand, every 1009th a wrapped
    one, every 4099th a pc outside the table."""
    r = np.arange(H, dtype=np.int64)
    pcs = np.where(r % 64 < 40, (r // 64 * 3) % T, (r * 7) % T)
    main, prep = clean(pcs, T)
    f = main[0].astype(np.int64)
    f[996::997, 1] = (f[996::997, 1] + 3) % P
    f[1008::1009, 2] = (f[1008::1009, 2] + TWO32) % P
    f[4098::4099, 0] = T + 5
    main[0] = f.astype(np.uint32)
    return main, prep


# ---- the BasicMachine's witnesses ---------------------------------------------------------------------------------------------------------
VM = {"fib25": lambda: va.Workload.fib(25), "fib582": lambda: va.Workload.fib(582), "alu100": lambda: va.Workload.alu(100),
      "signed_inequality": lambda: va.Workload.named("signed_inequality"), "left_imm_ops": lambda: va.Workload.named("left_imm_ops"), "loadfp": lambda: va.Workload.named("loadfp"),
      "static_data": lambda: va.Workload.named("static_data"), "mixed_ops8": lambda: va.Workload.named("mixed_ops:8")}
_witness = {}


def workload(name):
    if name not in _witness:
        w = VM[name]()
        _witness[name] = (w, w.main_traces(), w.preprocessed(), w.program_len)
    return _witness[name][0]


def witness(name):
    """(main traces, preprocessed, rom_len)"""
    workload(name)
    return _witness[name][1:]


def vm_tampered(kind):
    """fib(25) tampered (TAMPERINGS): operand a is cpu column 4, pc column 1; rom_len 23, the table's row 31 is padding."""
    main, prep, rom_len = witness("fib25")
    pc = int(main[CPU][100, 1])
    return tamper(main, prep, kind, CPU, 1, 4, PROGRAM, 0, 0, other_pc=(pc + 9) % rom_len) + (rom_len,)
