"""Inputs the memory audit's CPU and GPU tests share: the captured one-chip `ram` machine (columns is_read, clk, addr, is_static, v0..v3,
is_write; one receive on global bus 2 of the eight bare fields with count is_read + is_write), a two-receive variant (the second record of a row
in columns 9..17), the VM witnesses of the BasicMachine, the tampered fib(25) traces, and the edge traces, all built in numpy with fixed seeds."""
import numpy as np

import valida_amd as va
import valida_programs as vp
from domain_audit_cases import capture

P = va.P
MEM = 2
BUS = 2
IS_READ, CLK, ADDR, IS_STATIC, V0, IS_WRITE, WIDTH = 0, 1, 2, 3, 4, 8, 9
HEIGHTS = (1, 2, 64, 256, 512, 4096, 8192)
PLANT_POSITIONS = (63, 64, 65, 255, 256, 257, 2047, 2048, 4095, 4096, 4097)


def _receive(base, bus=BUS, fields=8):
    return (False, True, bus, [[(base + k, 1)] for k in range(fields)], [(base + IS_READ, 1), (base + IS_WRITE, 1)])


def ram_machine(bus=BUS, fields=8):
    return capture([(b"ram", WIDTH, [_receive(0, bus, fields)])])


def ram2_machine():
    """Two receives per row: seq order runs across the interactions of a row."""
    return capture([(b"ram2", 2 * WIDTH, [_receive(0), _receive(WIDTH)])])


def no_receive_machine():
    """The chip only SENDS on bus 2: there is no memory table."""
    return capture([(b"tx", WIDTH, [(True, True, BUS, [[(k, 1)] for k in range(8)], [(IS_READ, 1)])])])


def trace(n, records, width=WIDTH):
    """n rows (a power of two), dead but for records = [(row, is_read, clk, addr, is_static, value, is_write)] (value: an int for v3 or 4 values;
    is_write defaults to 1 - is_read: count 1)."""
    t = np.zeros((n, width), dtype=np.uint32)
    for rec in records:
        row, is_read, clk, addr, is_static, value = rec[:6]
        v = [0, 0, 0, value] if isinstance(value, (int, np.integer)) else list(value)
        t[row, :9] = [is_read % P, clk % P, addr % P, is_static % P] + [x % P for x in v] + [(rec[6] if len(rec) > 6 else 1 - is_read) % P]
    return t


def write(row, clk, addr, value):
    return (row, 0, clk, addr, 0, value)


def read(row, clk, addr, value):
    return (row, 1, clk, addr, 0, value)


def static(row, addr, value, clk=0):
    return (row, 0, clk, addr, 1, value)


def edge_traces():
    """[(name, trace)] at every height of HEIGHTS."""
    out = []
    for n in HEIGHTS:
        r = np.arange(n)
        out.append(("n%d_all_dead" % n, trace(n, [])))
        out.append(("n%d_one_write" % n, trace(n, [write(n - 1, 5, 100, 9)])))
        out.append(("n%d_one_read_of_0" % n, trace(n, [read(n // 2, 5, 100, 0)])))
        out.append(("n%d_one_read_of_7" % n, trace(n, [read(0, 5, 100, 7)])))
        out.append(("n%d_alternating" % n, trace(n, [write(k, k, 40, k // 2 % 256) if k % 2 == 0 else read(k, k, 40, k // 2 % 256) for k in r])))
        out.append(("n%d_own_address" % n, trace(n, [read(k, 3, 8 * int(k) + 4, k % 2) if k % 3 else write(k, 3, 8 * int(k) + 4, 1) for k in r])))
    return out


def planted(position, n=8192):
    """One address, the records at clk = their order position on the row of the same number: writes of k % 251 on every 7th position, reads of the
    last write between them; the read at `position` returns a wrong value.  Its last write lies up to six positions before it: for the
    positions of PLANT_POSITIONS in another wave, workgroup, scan block and sort block."""
    recs, last = [], 0
    for k in range(n):
        if k % 7 == 0 and k != position:
            last = k % 251
            recs.append(write(k, k, 77, last))
        else:
            recs.append(read(k, k, 77, last if k != position else (last + 1) % 256))
    return trace(n, recs)


def long_run(n=4096, run=3000):
    """A write, `run` reads of it, and a read that returns another value: the last write lies `run` + 1 positions back, across scan blocks.
    The second address before it keeps the run off position 0."""
    recs = [write(0, 1, 8, 3), read(1, 2, 8, 3), write(2, 1, 16, 200)] + [read(3 + k, 2 + k, 16, 200) for k in range(run)] + [read(3 + run, 2 + run, 16, 201)]
    return trace(n, recs), 3 + run


def permuted(t, seed=11):
    """The same records on other rows (a fixed permutation): row[i] of the result is row perm[i] of t."""
    perm = np.random.RandomState(seed).permutation(t.shape[0])
    return t[perm], perm


def same_cycle(read_first):
    """A write of 5 at clk 3, then at clk 9 a read of 6 and a write of 6 in one cycle: clean when the write comes first in the trace."""
    a, b = (read(2, 9, 24, 6), write(3, 9, 24, 6)) if read_first else (write(2, 9, 24, 6), read(3, 9, 24, 6))
    return trace(4, [write(0, 3, 24, 5), a, b])


def static_traces():
    return [("before_reads", trace(8, [static(0, 12, 33), read(1, 4, 12, 33), read(5, 9, 12, 33), static(6, 20, 1)])),
            ("duplicate", trace(8, [static(0, 12, 33), static(1, 12, 34), read(2, 4, 12, 34)])),
            ("clk_not_0", trace(8, [static(0, 12, 33, clk=2), read(1, 4, 12, 33)])),
            ("beside_an_operation_at_clk_0", trace(8, [write(0, 0, 12, 8), static(3, 12, 33), read(4, 0, 12, 8)])),
            ("static_read", trace(8, [(0, 1, 0, 12, 1, 0, 0)]))]


def extreme_traces():
    top = [write(k, 1, (k % 4) << 24, 1) for k in range(64)] + [read(64 + k, 2, (k % 4) << 24, 1) for k in range(64)]
    return [("addr_clk_0_and_p_minus_1", trace(8, [write(0, 0, 0, 1), read(1, P - 1, 0, 1), write(2, 0, P - 1, 2), read(3, P - 1, P - 1, 2), read(4, P - 1, P - 1, 3)])),
            ("top_byte_of_addr_varies", trace(128, top)),
            ("no_byte_varies", trace(64, [write(k, 6, 0x01020304, 9) for k in range(64)])),
            ("no_byte_varies_all_live_reads", trace(64, [read(k, 6, 0x01020304, 0) for k in range(64)])),
            ("values_256_and_p_minus_1", trace(8, [write(0, 1, 4, [0, 0, 0, 256]), read(1, 2, 4, [0, 0, 0, 256]), write(2, 3, 4, [P - 1, 0, 0, 0]), read(3, 4, 4, [P - 1, 0, 0, 1])])),
            ("count_2_and_is_read_2", trace(8, [(0, 1, 1, 4, 0, 0, 1), (1, 2, 2, 4, 0, 5, P - 1), read(2, 3, 4, 5), (3, 0, 4, 4, 2, 6), read(4, 5, 4, 6)])),
            ("clk_gap_and_addr_gap_above_L", trace(8, [write(0, 1, 4, 1), read(1, 100, 4, 1), write(2, 7, 1000, 2), read(3, 8, 1000, 2), read(4, 8 + 4, 1000, 2)]))]


def many_findings(n=512, k=300):
    """k reads of a non-zero value at addresses nobody writes."""
    return trace(n, [read(r, 1, 4 * r, 1 + r % 255) for r in range(k)])


def two_receive_trace(n=64, seed=5):
    """ram2: both records of a row at one (addr, clk): the write in interaction 0 and the read of it in interaction 1 on even rows, the read first
    (stale) on the rows divisible by 8."""
    t = np.zeros((n, 2 * WIDTH), dtype=np.uint32)
    rs = np.random.RandomState(seed)
    for r in range(0, n, 2):
        v = int(rs.randint(1, 256))
        w = [0, r, 4 * (r % 6), 0, 0, 0, 0, v, 1]
        rd = [1, r, 4 * (r % 6), 0, 0, 0, 0, v, 0]
        t[r] = (rd + w) if r % 8 == 0 else (w + rd)
    return t


def synthetic(n, seed=3, addresses=257, stale_every=997):
    """n records (every row live) of `addresses` addresses, clk = row: consistent writes and reads, but every `stale_every`-th row a stale read."""
    rs = np.random.RandomState(seed)
    addr = rs.randint(0, addresses, size=n).astype(np.int64)
    is_read = (rs.randint(0, 4, size=n) != 0).astype(np.int64)
    val = rs.randint(1, 256, size=n).astype(np.int64)
    order = np.lexsort((np.arange(n), addr))
    a, w, v, pos = addr[order], 1 - is_read[order], val[order], np.arange(n)
    first = np.r_[True, a[1:] != a[:-1]]
    last = np.maximum.accumulate(np.where(w == 1, pos, -1))  # the last write at or before a position
    has = last >= np.maximum.accumulate(np.where(first, pos, 0))  # .. if it belongs to this address
    value = np.where(w == 1, v, np.where(has, v[np.maximum(last, 0)], 0))
    out_val = np.empty(n, dtype=np.int64)
    out_val[order] = value
    rows = np.arange(n)
    stale = (rows % stale_every == stale_every - 1) & (is_read == 1)
    out_val = np.where(stale, (out_val + 1) % 256, out_val)
    t = np.zeros((n, WIDTH), dtype=np.uint32)
    t[:, IS_READ], t[:, CLK], t[:, ADDR], t[:, V0 + 3], t[:, IS_WRITE] = is_read, rows, 8 * addr, out_val, 1 - is_read
    return t


# ---- the BasicMachine's witnesses ---------------------------------------------------------------------------------------------------------
VM = {"fib25": lambda: va.Workload.fib(25), "alu50": lambda: va.Workload.alu(50), "fib582": lambda: va.Workload.fib(582),
      "left_imm_ops": lambda: va.Workload.named("left_imm_ops"), "signed_inequality": lambda: va.Workload.named("signed_inequality"), "loadfp": lambda: va.Workload.named("loadfp"),
      "mixed_ops20": lambda: va.Workload.named("mixed_ops:20"), "static_data": lambda: va.Workload.named("static_data"),
      "byte_loads": lambda: va.Workload.from_executable(vp.machine_code(vp.byte_loads_program())),
      "store_byte": lambda: va.Workload.from_executable(vp.machine_code(vp.store_byte_program()))}
_witness = {}


def witness(name):
    if name not in _witness:
        w = VM[name]()
        _witness[name] = (w.main_traces(), w.preprocessed())
    return _witness[name]


def tampered(kind):
    """fib(25) with its mem trace tampered: (main traces, preprocessed, the tampered mem row).  'read': one read's low value byte changed;
    'write': one write's (a write that reads follow); 'uninit': a read moved to an address nobody writes, its value non-zero."""
    import memory_audit_ref as ref

    mt, prep = witness("fib25")
    mt = [m.copy() for m in mt]
    machine = va.Machine.basic()
    rec, _, _, _ = ref.records(machine, mt, prep)
    bare = [f[1][0][1] for f in machine.interactions(MEM)[0]["fields"]]  # the fields of mem's receive are bare columns
    assert all(f[0] == 0 and len(f[1]) == 1 and f[1][0][2] == 1 for f in machine.interactions(MEM)[0]["fields"])
    reads, writes = [int(r[1]) for r in rec if r[4] == 1], [int(r[1]) for r in rec if r[4] == 0]
    t = mt[MEM]
    if kind == "read":
        row = reads[len(reads) // 2]
        t[row, bare[7]] = (int(t[row, bare[7]]) + 1) % 256
    elif kind == "write":
        row = writes[len(writes) // 3]
        t[row, bare[7]] = (int(t[row, bare[7]]) + 1) % 256
    else:
        row = reads[len(reads) // 2]
        t[row, bare[2]] = 40000
        t[row, bare[7]] = 9
    return mt, prep, row
