"""Inputs the domain audit's CPU and GPU tests share: the captured "needle" machine (a chip whose byte column is bare-sent to a one-chip table
bus under a gate column, and the table chip), the captured three-column "edge" AIR with one send whose second field is not bare, and the edge
traces: small heights, value sets at the class and bitmap-word boundaries, patterns that switch at rows 63 / 64 / 65 / 255 / 256 / 257 (a wave,
a tile and one row to either side; heights themselves are powers of two by the machine's rule), all 65536 narrow values, a constant and an
alternating column."""
import ctypes

import numpy as np

import valida_amd as va

P = va.P
NEEDLE_N, NEEDLE_BUS = 512, 5


class VcolTerm(ctypes.Structure):  # vgpu_vcol_term_t
    _fields_ = [("is_preprocessed", ctypes.c_uint32), ("column", ctypes.c_uint32), ("weight", ctypes.c_uint32)]


class Vcol(ctypes.Structure):  # vgpu_vcol_t
    _fields_ = [("terms", ctypes.POINTER(VcolTerm)), ("n_terms", ctypes.c_uint32), ("constant", ctypes.c_uint32)]


class Interaction(ctypes.Structure):  # vgpu_interaction_t
    _fields_ = [("fields", ctypes.POINTER(Vcol)), ("n_fields", ctypes.c_uint32), ("count", Vcol), ("is_global", ctypes.c_uint32), ("bus_index", ctypes.c_uint32),
                ("is_send", ctypes.c_uint32)]


def _vcol(terms, constant=0):
    arr = (VcolTerm * max(1, len(terms)))(*[VcolTerm(0, c, w) for c, w in terms])
    v = Vcol(arr, len(terms), constant)
    v._keep = arr
    return v


def capture(chips):
    """A machine of captured AIRs without constraints: chips = [(name, width, [(is_send, is_global, bus, [field terms, ..], count terms)])],
    a vcol given as a list of (column, weight), optionally (terms, constant)."""
    L, u = va.lib(), ctypes.c_uint32
    L.vgpu_air_add_interaction.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    m = ctypes.c_void_p()
    assert L.vgpu_machine_new(ctypes.byref(m)) == 0

    def vc(x):
        return _vcol(*x) if isinstance(x, tuple) else _vcol(x)

    for name, width, interactions in chips:
        air = ctypes.c_void_p()
        assert L.vgpu_air_new(name, u(width), u(0), ctypes.byref(air)) == 0
        for is_send, is_global, bus, fields, count in interactions:
            fs = [vc(f) for f in fields]
            arr = (Vcol * len(fs))(*fs)
            it = Interaction(arr, len(fs), vc(count), int(is_global), bus, int(is_send))
            assert L.vgpu_air_add_interaction(air, ctypes.byref(it)) == 0, L.vgpu_last_error()
        assert L.vgpu_machine_push_air(m, air) == 0, L.vgpu_last_error()
        L.vgpu_air_free(air)
    return va.Machine(m)


def needle_machine(bus=NEEDLE_BUS):
    """user (b, g, x): sends (b) with count g to global bus `bus`; table (v, mult): receives (v) with count mult.  The table chip has no
    constraint and no send: the bus is a lookup bus by the structural rule."""
    return capture([(b"user", 3, [(True, True, bus, [[(0, 1)]], [(1, 1)])]), (b"table", 2, [(False, True, bus, [[(0, 1)]], [(1, 1)])])])


def needle_traces(broken):
    """512 rows: b = 1 + r mod 255 (never zero), g = 1 on every row (broken: but row 511), x = r^2 (wide); the table offers 0 .. 255."""
    r = np.arange(NEEDLE_N, dtype=np.uint64)
    g = np.ones(NEEDLE_N, dtype=np.uint64)
    if broken:
        g[NEEDLE_N - 1] = 0
    user = np.stack([1 + r % 255, g, r * r % P], axis=1).astype(np.uint32)
    table = np.stack([np.arange(256), np.bincount(user[g == 1, 0], minlength=256)], axis=1).astype(np.uint32)
    return [user, table]


def edge_machine():
    """edge (a, m, r): one send on global bus 0 (nobody receives: not a lookup bus) of (a, 2 a + r + 7) with count m."""
    return capture([(b"edge", 3, [(True, True, 0, [[(0, 1)], ([(0, 2), (2, 1)], 7)], [(1, 1)])])])


def _pattern(values, n, switch=None):
    """n rows cycling through `values`; from row `switch` on the values are doubled-plus-one mod p (another set)."""
    v = np.array([values[k % len(values)] for k in range(n)], dtype=np.uint64)
    if switch is not None:
        v[switch:] = (2 * v[switch:] + 1) % P
    return v


VALUE_SETS = [[0], [0, 1], [255], [256], [31, 32], [65535], [65536], [P - 1]]


def edge_traces():
    """[(name, trace)]: column a holds the pattern, column m a gate (1, but 0 on every third row; on one-row traces 1), column r the row."""
    out = []

    def add(name, a, m=None):
        n = len(a)
        r = np.arange(n, dtype=np.uint64)
        gate = (r % 3 != 2).astype(np.uint64) if m is None else m
        out.append((name, np.stack([a % P, gate, r], axis=1).astype(np.uint32)))

    for n in (1, 2, 64, 256, 512):
        for vs in VALUE_SETS:
            add("n%d_%s" % (n, "_".join(str(v) for v in vs)), _pattern(vs, n))
    for k in (63, 64, 65, 255, 256, 257):  # the pattern switches at row k of a trace of 512 rows: inside a wave, at its end, one row into the next; the same for a tile
        add("switch%d_const" % k, _pattern([200], 512, k))
        add("switch%d_bytes" % k, _pattern([3, 250, 17], 512, k), m=(np.arange(512) >= k).astype(np.uint64))
    add("constant", _pattern([77], 1024), m=np.ones(1024, dtype=np.uint64))
    add("alternating", _pattern([5, 300], 1024))
    add("live_nowhere", _pattern([9, 10], 256), m=np.zeros(256, dtype=np.uint64))
    return out


def all_narrow_values():
    """65536 rows: a is a fixed permutation of 0 .. 65535 (dense, 65536 distinct values), m = 1."""
    a = np.random.RandomState(7).permutation(65536).astype(np.uint64)
    return np.stack([a, np.ones(65536, dtype=np.uint64), np.arange(65536, dtype=np.uint64)], axis=1).astype(np.uint32)
