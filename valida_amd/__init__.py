"""valida_amd — MI355X-native STARK prover backend for the Valida zkVM (hot path: Machine::prove).

This package is a thin ctypes mirror of the C ABI in include/vgpu.h (libvgpu.so: hand-written
HIP/gfx950 kernels + C++ host prover).  Names follow the reference's own surface for this path:
`Machine.prove`, `Pcs.commit_batches` / `get_ldes`, `generate_permutation_trace`, `Challenger`.
There is NO CPU fallback: constructing a `Prover` without a HIP device raises `VgpuError`.
"""
import ctypes
import os

import numpy as np

P = 2013265921
NUM_CHIPS = 14
CHIP_NAMES = ["cpu", "program", "mem", "add", "sub", "mul", "div", "shift", "lt", "com", "bitwise", "output", "range", "static_data"]

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.environ.get("VGPU_LIB_PATH") or os.path.join(_HERE, "libvgpu.so")  # the override serves A/B runs of two builds in one session

c_u32p = ctypes.POINTER(ctypes.c_uint32)
c_u64p = ctypes.POINTER(ctypes.c_uint64)


HASH_KECCAK256, HASH_POSEIDON16 = 0, 1  # vgpu_config.hash_kind


class VgpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("vgpu error %d: %s" % (code, msg))
        self.code = code


class VgpuConfig(ctypes.Structure):
    _fields_ = [
        ("device", ctypes.c_int32),
        ("log_blowup", ctypes.c_uint32),
        ("num_queries", ctypes.c_uint32),
        ("pow_bits", ctypes.c_uint32),
        ("hash_kind", ctypes.c_uint32),
        ("observe_final_poly", ctypes.c_uint32),
        ("poseidon_rc", ctypes.c_uint32 * 480),
        ("interpret_air", ctypes.c_uint32),
    ]


_lib = None


def lib():
    """Load libvgpu.so (built in-tree by valida_amd/build.py).  Fails loudly if it is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise ImportError("libvgpu.so is not built: run `python valida_amd/build.py` (or __graft_entry__.build())")
        L = ctypes.CDLL(_LIB_PATH)
        L.vgpu_last_error.restype = ctypes.c_char_p
        L.vgpu_version.restype = ctypes.c_char_p
        L.vgpu_proof_len.restype = ctypes.c_uint64
        L.vgpu_proof_words.restype = c_u32p
        L.vgpu_challenger_sample_bits.restype = ctypes.c_uint64
        L.vgpu_proof_debug_perm_trace.restype = ctypes.c_int64
        L.vgpu_proof_debug_quotient.restype = ctypes.c_int64
        L.vgpu_prover_profile.restype = ctypes.c_int64
        L.vgpu_verifier_message.restype = ctypes.c_int64
        L.vgpu_verifier_message.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64]
        L.vgpu_verifier_timing.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.vgpu_verifier_timing.restype = None
        L.vgpu_shader_clock_probe.argtypes = [ctypes.c_int32, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
        L.vgpu_shader_clock_probe.restype = ctypes.c_int32
        L.vgpu_workload_from_executable.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64,
                                                    ctypes.POINTER(ctypes.c_void_p)]
        L.vgpu_workload_output.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64]
        L.vgpu_workload_output.restype = ctypes.c_int64
        for name in ("vgpu_air_constant", "vgpu_air_variable", "vgpu_air_is_first_row", "vgpu_air_is_last_row", "vgpu_air_is_transition", "vgpu_air_add",
                     "vgpu_air_sub", "vgpu_air_mul", "vgpu_air_neg", "vgpu_machine_num_chips", "vgpu_challenger_grind"):
            getattr(L, name).restype = ctypes.c_uint32
        _lib = L
    return _lib


def _check(code):
    if code != 0:
        raise VgpuError(code, lib().vgpu_last_error().decode())


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(c_u32p)


def shader_clock_hz(device=0, iters=8192):
    """The shader clock the device sustains right now (vgpu_shader_clock_probe: one wave, a chain of `iters` VALU additions, shader cycles
    against the 100 MHz wall clock).  Safe beside running proofs; bench.py samples it over its timed region."""
    out = (ctypes.c_uint64 * 2)()
    _check(lib().vgpu_shader_clock_probe(ctypes.c_int32(device), ctypes.c_uint32(iters), out))
    return float(out[0]) / float(out[1]) * 1e8


def poseidon_round_constants(seed=0x56414C494441, source="splitmix", **cli_switches):
    """480 Poseidon-16 round constants from SplitMix64(seed), rejection-sampled 31-bit values < p.

    The reference draws them from thread_rng (basic/tests/test_prover.rs:422); they are configuration
    input here — the same array must be given to the prover and the verifier.
    source="cli": the constants of the reference's CLI instead — Pcg64 seeded by Seeder::from("validia seed")
    (basic/src/bin/valida.rs:364-365), restated in valida_amd/cli_constants.py (switches: raw_monty, sip_adj0).
    """
    if source == "cli":
        from .cli_constants import cli_poseidon_round_constants

        return cli_poseidon_round_constants(**cli_switches)
    if source != "splitmix":
        raise ValueError("source must be 'splitmix' or 'cli'")
    out = []
    x = seed & 0xFFFFFFFFFFFFFFFF
    while len(out) < 480:
        x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
        z ^= z >> 31
        v = (z >> 33) & 0x7FFFFFFF
        if v < P:
            out.append(v)
    return np.array(out, dtype=np.uint32)


class OplogDesc(ctypes.Structure):  # vgpu_oplog_desc_t
    _fields_ = [
        ("struct_size", ctypes.c_uint64),  # = sizeof(vgpu_oplog_desc_t); vgpu_workload_oplog fills it in
        ("cpu", ctypes.c_void_p), ("n_cpu", ctypes.c_uint64),
        ("mem", ctypes.c_void_p), ("n_mem", ctypes.c_uint64),
        ("alu", ctypes.c_void_p * 4), ("n_alu", ctypes.c_uint64 * 4),
        ("static_cells", ctypes.c_void_p), ("n_static", ctypes.c_uint64),
        ("rom_len", ctypes.c_uint32),
        ("alu2", ctypes.c_void_p * 4), ("n_alu2", ctypes.c_uint64 * 4),  # mul, div, shift, com
        ("output", ctypes.c_void_p), ("n_output", ctypes.c_uint64),      # OutputChip::values as (clk, byte)
    ]


def decode_interaction_words(w):
    """Inverse of the neutral interaction word image (vgpu_machine_interaction_words)."""
    w = [int(x) for x in w]
    pos = 1

    def vcol():
        nonlocal pos
        nt, const = w[pos], w[pos + 1]
        pos += 2
        terms = []
        for _ in range(nt):
            terms.append((w[pos], w[pos + 1], w[pos + 2]))
            pos += 3
        return (const, terms)

    out = []
    for _ in range(w[0]):
        send, glob, bus, nf = w[pos:pos + 4]
        pos += 4
        count = vcol()
        out.append({"send": bool(send), "global": bool(glob), "bus": bus, "count": count, "fields": [vcol() for _ in range(nf)]})
    assert pos == len(w)
    return out


GENERATED_CHIPS = tuple(range(14))  # every BasicMachine chip has a log-driven device trace generator


def validate_oplog(desc):
    """The checks Prover.upload_oplog makes before it touches the device (vgpu_oplog_validate); raises VgpuError with the reason."""
    _check(lib().vgpu_oplog_validate(ctypes.byref(desc)))


class Workload:
    """A program run on the BasicMachine, all chip traces generated (host): a built-in one (fib_program(n), ...) or a Valida executable."""

    def __init__(self, handle):
        self._h = handle
        st = (ctypes.c_uint64 * 8)()
        lib().vgpu_workload_stats(self._h, st)
        self.cycles, self.cpu_ops, self.mem_ops, self.add_ops, self.result, self.program_len, self.cpu_height = [int(v) for v in st[:7]]

    @classmethod
    def fib(cls, n):
        h = ctypes.c_void_p()
        _check(lib().vgpu_workload_fib(ctypes.c_uint32(n), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def alu(cls, iters):
        """ALU-heavy loop (workload C4): 4 + 9 * iters + 1 cycles, exercising add / sub / bitwise / lt chips."""
        h = ctypes.c_void_p()
        _check(lib().vgpu_workload_alu(ctypes.c_uint32(iters), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def named(cls, name):
        """One of the reference's other pinned prover programs: left_imm_ops, signed_inequality, loadfp, static_data; or "mixed_ops[:iters]", the
        synthetic program that keeps every chip busy (mul, div, shift, com, output included)."""
        h = ctypes.c_void_p()
        _check(lib().vgpu_workload_named(name.encode(), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def from_executable(cls, data, advice=b"", stack_height=1 << 24, max_cycles=1 << 22):
        """A Valida executable — raw machine code (24-byte little-endian records) or a little-endian ELF — run as `valida run` runs it
        (basic/src/bin/valida.rs:340-354): fp = stack_height, the FixedAdviceProvider tape `advice`.  A run that has not stopped after
        max_cycles cycles is refused; max_cycles = 0 loads without running (ROM, static data, preprocessed traces only).  A file or program
        the loader or the VM refuses raises VgpuError with the reason."""
        data, advice = bytes(data), bytes(advice)
        h = ctypes.c_void_p()
        _check(lib().vgpu_workload_from_executable(data, len(data), stack_height, advice, len(advice), max_cycles, ctypes.byref(h)))
        return cls(h)

    def output(self):
        """OutputChip::bytes (output/src/lib.rs:27-29): what the program WROTE, as bytes."""
        n = lib().vgpu_workload_output(self._h, None, 0)
        if n < 0:
            _check(int(n))
        buf = ctypes.create_string_buffer(max(1, int(n)))
        lib().vgpu_workload_output(self._h, buf, n)
        return buf.raw[:n]

    def cell(self, addr):
        v = ctypes.c_uint32()
        _check(lib().vgpu_workload_cell(self._h, ctypes.c_uint32(addr), ctypes.byref(v)))
        return int(v.value)

    def main_trace(self, chip):
        data, h, w = c_u32p(), ctypes.c_uint64(), ctypes.c_uint64()
        _check(lib().vgpu_workload_main_trace(self._h, ctypes.c_uint32(chip), ctypes.byref(data), ctypes.byref(h), ctypes.byref(w)))
        return np.ctypeslib.as_array(data, shape=(h.value, w.value)).copy()  # the workload owns the buffer

    def main_traces(self):
        return [self.main_trace(i) for i in range(NUM_CHIPS)]

    def oplog(self):
        """The VM's operation logs (vgpu_oplog_desc_t; buffers owned by this workload)."""
        d = OplogDesc()
        lib().vgpu_workload_oplog(self._h, ctypes.byref(d))
        d._owner = self
        return d

    def preprocessed(self):
        """[(chip index, matrix)] in chip order: program ROM, range table."""
        out = []
        for k in range(2):
            chip, data, h, w = ctypes.c_uint32(), c_u32p(), ctypes.c_uint64(), ctypes.c_uint64()
            _check(lib().vgpu_workload_preprocessed(self._h, ctypes.c_uint32(k), ctypes.byref(chip), ctypes.byref(data), ctypes.byref(h), ctypes.byref(w)))
            out.append((chip.value, np.ctypeslib.as_array(data, shape=(h.value, w.value)).copy()))
        return out

    def program_audit_host(self, max_findings=64, max_ranges=64):
        """The host program audit of this workload's own witness with rom_len = program_len: the table's zero padding rows are not fetchable."""
        return program_audit_host(Machine.basic(), self.main_traces(), self.preprocessed(), rom_len=self.program_len, max_findings=max_findings, max_ranges=max_ranges)

    def arithmetic_audit_host(self, max_findings=64, sides="receives"):
        """The host arithmetic audit of this workload's own witness: the general bus's records recomputed as 32-bit arithmetic."""
        return arithmetic_audit_host(Machine.basic(), self.main_traces(), self.preprocessed(), max_findings=max_findings, sides=sides)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_workload_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


class Machine:
    """Ordered chips with compiled constraint programs (basic/src/lib.rs:151-166)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def basic(cls):
        h = ctypes.c_void_p()
        _check(lib().vgpu_machine_basic(ctypes.byref(h)))
        return cls(h)

    @classmethod
    def basic_via_ffi(cls):
        """The same chips captured through the vgpu_air_* FFI (what a foreign host does): interpreted AIR programs."""
        h = ctypes.c_void_p()
        _check(lib().vgpu_machine_basic_via_ffi(ctypes.byref(h)))
        return cls(h)

    @property
    def num_chips(self):
        return int(lib().vgpu_machine_num_chips(self._h))

    def chip_info(self, chip):
        out = (ctypes.c_uint32 * 8)()
        _check(lib().vgpu_machine_chip_info(self._h, ctypes.c_uint32(chip), out))
        keys = ["width", "preprocessed_width", "interactions", "log_quotient_degree", "constraints", "instructions", "registers", "max_degree"]
        return dict(zip(keys, [int(v) for v in out]))

    def interactions(self, chip):
        """Chip::all_interactions of `chip` as a list of dicts (send, global, bus, count, fields); a virtual column is
        (constant, [(is_preprocessed, column, weight), ...])."""
        L = lib()
        L.vgpu_machine_interaction_words.restype = ctypes.c_int64
        n = L.vgpu_machine_interaction_words(self._h, ctypes.c_uint32(chip), None, ctypes.c_uint64(0))
        if n < 0:
            _check(int(n))
        w = np.zeros(int(n), dtype=np.uint32)
        L.vgpu_machine_interaction_words(self._h, ctypes.c_uint32(chip), w.ctypes.data_as(c_u32p), ctypes.c_uint64(w.size))
        return decode_interaction_words(w)

    def eval_constraints(self, chip, main_local, main_next, prep_local=None, prep_next=None, is_first=0, is_last=0, is_transition=1):
        info = self.chip_info(chip)
        pl = np.zeros(max(1, info["preprocessed_width"]), dtype=np.uint32) if prep_local is None else prep_local
        pn = np.zeros(max(1, info["preprocessed_width"]), dtype=np.uint32) if prep_next is None else prep_next
        a, ap = _u32(main_local)
        b, bp = _u32(main_next)
        c, cp = _u32(pl)
        d, dp = _u32(pn)
        out = np.zeros(max(1, info["constraints"]), dtype=np.uint32)
        n = lib().vgpu_machine_eval_constraints(self._h, ctypes.c_uint32(chip), ap, bp, cp, dp, ctypes.c_uint32(is_first), ctypes.c_uint32(is_last),
                                                ctypes.c_uint32(is_transition), out.ctypes.data_as(c_u32p), ctypes.c_uint32(out.size))
        if n < 0:
            _check(n)
        return out[:n]

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_machine_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


class Challenger:
    """DuplexChallenger<BabyBear, Poseidon16, 16> (host)."""

    def __init__(self, rc):
        self._rc, rcp = _u32(rc)
        self._h = ctypes.c_void_p()
        _check(lib().vgpu_challenger_new(rcp, ctypes.byref(self._h)))

    def observe(self, values):
        v, vp = _u32(values)
        lib().vgpu_challenger_observe(self._h, vp, ctypes.c_uint64(v.size))

    def sample(self, n=1):
        out = np.zeros(n, dtype=np.uint32)
        lib().vgpu_challenger_sample(self._h, out.ctypes.data_as(c_u32p), ctypes.c_uint64(n))
        return out

    def sample_bits(self, bits):
        return int(lib().vgpu_challenger_sample_bits(self._h, ctypes.c_uint32(bits)))

    def grind(self, bits):
        return int(lib().vgpu_challenger_grind(self._h, ctypes.c_uint32(bits)))

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_challenger_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


def poseidon16_permute(rc, state):
    r, rp = _u32(rc)
    s = np.array(state, dtype=np.uint32)
    lib().vgpu_poseidon16_permute(rp, s.ctypes.data_as(c_u32p))
    return s


# vgpu_field_probe: op name -> (op code, operand words per item, result words per item), in the order of vk::FieldProbeOp (kernels/launch.hpp).
# The butterfly ops take 16 points, low, lowbits; monty_reduce / monty_reduce_wide / monty_signed take the 64-bit operand as (low word, high word).
FIELD_PROBE_OPS = {name: (code, iw, ow) for code, (name, iw, ow) in enumerate([
    ("reduce_once", 1, 1), ("sub_mod", 2, 1), ("add", 2, 1), ("sub", 2, 1), ("neg", 1, 1), ("mul", 2, 1), ("monty_reduce", 2, 1), ("monty_reduce_wide", 2, 1),
    ("from_canonical", 1, 1), ("canonical", 1, 1), ("inv", 1, 1), ("ext_mul", 10, 5), ("ext_square", 5, 5), ("ext_scale", 6, 5), ("ext_inv", 5, 5),
    ("bfly_dit_lb0", 18, 16), ("bfly_dit", 18, 16), ("bfly_dif_lb0", 18, 16), ("bfly_dif", 18, 16), ("monty_signed", 2, 1), ("sbox", 1, 1), ("sbox_plus", 2, 1),
    ("permute", 16, 16), ("permute_plain", 16, 16)])}


def field_probe(prover, op, operands):
    """Test hook (vgpu_field_probe): primitive `op` (a key of FIELD_PROBE_OPS) of the DEVICE's field arithmetic on operands[i] = one item's raw
    stored words, one work item each -> (n_items, result words) raw stored words.  Nothing is converted on the way in or out."""
    code, iw, ow = FIELD_PROBE_OPS[op]
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != iw or a.shape[0] == 0:
        raise ValueError("field_probe(%s): operands must be a non-empty (n_items, %d) array" % (op, iw))
    n = a.shape[0]
    src = np.ascontiguousarray(a.T)
    out = np.zeros((ow, n), dtype=np.uint32)
    _check(lib().vgpu_field_probe(prover._h, ctypes.c_uint32(code), src.ctypes.data_as(c_u32p), ctypes.c_uint64(src.size), ctypes.c_uint64(n),
                                  out.ctypes.data_as(c_u32p), ctypes.c_uint64(out.size)))
    return np.ascontiguousarray(out.T)


# vgpu_lazy_probe: op name -> (op code, operand words per item as a function of the sum's length, result words per item, the lengths the op is built
# for; (0,) = the op has no length).  In the order of vk::LazyProbeOp (kernels/launch.hpp); a list of its own beside FIELD_PROBE_OPS.
LAZY_PROBE_OPS = {name: (code, iw, ow, tuple(terms)) for code, (name, iw, ow, terms) in enumerate([
    ("fold_hi", lambda n: 2, 2, (0,)), ("ext_mul", lambda n: 10, 5, (0,)), ("lin_dot", lambda n: 6 * n, 5, list(range(1, 18)) + [34]),
    ("ext_dot", lambda n: 10 * n, 5, range(1, 9)), ("lin_dot_loop", lambda n: 6 * n, 5, range(1, 65))])}


def lazy_probe(prover, op, terms, operands):
    """Test hook (vgpu_lazy_probe): fold_hi, the Ext5 product or a lazily folded sum of `terms` terms (a key of LAZY_PROBE_OPS; terms = 0 where the op
    has none) of the DEVICE's field arithmetic on operands[i] = one item's raw stored words -> (n_items, result words) raw stored words."""
    code, iwf, ow, lengths = LAZY_PROBE_OPS[op]
    if terms not in lengths:
        raise ValueError("lazy_probe(%s): no such length %r" % (op, terms))
    iw = iwf(terms)
    a = np.ascontiguousarray(operands, dtype=np.uint32)
    if a.ndim != 2 or a.shape[1] != iw or a.shape[0] == 0:
        raise ValueError("lazy_probe(%s, %d): operands must be a non-empty (n_items, %d) array" % (op, terms, iw))
    n = a.shape[0]
    src = np.ascontiguousarray(a.T)
    out = np.zeros((ow, n), dtype=np.uint32)
    _check(lib().vgpu_lazy_probe(prover._h, ctypes.c_uint32(code), ctypes.c_uint32(terms), src.ctypes.data_as(c_u32p), ctypes.c_uint64(src.size), ctypes.c_uint64(n),
                                 out.ctypes.data_as(c_u32p), ctypes.c_uint64(out.size)))
    return np.ascontiguousarray(out.T)


class _PinnedBlock:
    def __init__(self, nbytes):
        self.ptr = ctypes.c_void_p()
        _check(lib().vgpu_host_alloc(ctypes.c_uint64(max(1, nbytes)), ctypes.byref(self.ptr)))

    def __del__(self):
        if getattr(self, "ptr", None):
            try:
                lib().vgpu_host_free(self.ptr)
            except TypeError:  # interpreter shutdown
                pass
            self.ptr = None


def pinned_empty(shape, dtype=np.uint32):
    """numpy array in page-locked host memory (vgpu_host_alloc): uploads from it are plain DMA.  The memory lives as long as the array
    (or any view of it) does."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    dt = np.dtype(dtype)
    n = int(np.prod(shape)) if shape else 1
    blk = _PinnedBlock(n * dt.itemsize)
    buf = (ctypes.c_char * max(1, n * dt.itemsize)).from_address(blk.ptr.value)
    buf._vgpu_block = blk  # the ctypes buffer (numpy's .base) keeps the allocation alive
    return np.frombuffer(buf, dtype=dt, count=n).reshape(shape)


def pinned_copy(a):
    out = pinned_empty(a.shape, a.dtype)
    out[...] = a
    return out


class DeviceOplog:
    def __init__(self, prover, handle, nbytes):
        self._prover, self._h, self.nbytes = prover, handle, nbytes

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_oplog_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


class DeviceTrace:
    def __init__(self, prover, handle, shape):
        self._prover, self._h, self.shape = prover, handle, shape

    def download(self):
        """Canonical row-major copy (what the reference's generate_trace would have returned)."""
        out = np.zeros(self.shape, dtype=np.uint32)
        _check(lib().vgpu_trace_download(self._prover._h, self._h, out.ctypes.data_as(c_u32p), ctypes.c_uint64(out.size)))
        return out

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_trace_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


class ProverData:
    """Pcs::ProverData — committed LDEs + Merkle tree, resident in HBM."""

    def __init__(self, prover, handle, root, shapes):
        self._prover, self._h, self.root, self._shapes = prover, handle, root, shapes

    def lde(self, idx):
        """get_ldes()[idx] in committed (bit-reversed) row order, canonical values."""
        h, w = self._shapes[idx]
        H = h << self._prover.log_blowup
        out = np.zeros((H, w), dtype=np.uint32)
        _check(lib().vgpu_pdata_lde(self._prover._h, self._h, ctypes.c_uint32(idx), out.ctypes.data_as(c_u32p), ctypes.c_uint64(out.size)))
        return out

    def lde_view(self, idx):
        """pcs.get_ldes()[idx] without a copy: (device pointer, height, width, stride, log_blowup) of the committed LDE in HBM."""

        class _View(ctypes.Structure):  # vgpu_lde_view_t
            _fields_ = [("data", ctypes.c_void_p), ("height", ctypes.c_uint64), ("width", ctypes.c_uint64), ("stride", ctypes.c_uint64), ("log_blowup", ctypes.c_uint32)]

        v = _View()
        _check(lib().vgpu_pdata_lde_view(self._h, ctypes.c_uint32(idx), ctypes.byref(v)))
        return {"data": v.data, "height": int(v.height), "width": int(v.width), "stride": int(v.stride), "log_blowup": int(v.log_blowup)}

    @property
    def num_matrices(self):
        lib().vgpu_pdata_num_matrices.restype = ctypes.c_uint32
        return int(lib().vgpu_pdata_num_matrices(self._h))

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_pdata_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


class Proof:
    def __init__(self, handle):
        self._h = handle
        n = int(lib().vgpu_proof_len(handle))
        self.words = np.ctypeslib.as_array(lib().vgpu_proof_words(handle), shape=(n,)).copy()
        ms = (ctypes.c_double * 11)()
        lib().vgpu_proof_phase_ms(handle, ms)
        keys = ["ingest", "commit_main", "perm", "commit_perm", "quotient", "commit_quotient", "open_values", "open_reduce", "fri", "queries", "total"]
        self.phase_ms = dict(zip(keys, [float(v) for v in ms]))
        t = (ctypes.c_uint32 * 33)()
        lib().vgpu_proof_transcript(handle, t)
        self.transcript = np.array(t, dtype=np.uint32)

    def bytes(self):
        return self.words.tobytes()

    def cbor(self, flags=0):
        """The proof as the reference writes it to disk: CBOR of the serde-derived MachineProof (see proof_cbor)."""
        return proof_cbor(self.words, flags)

    def _dbg(self, fn, chip):
        n = fn(self._h, ctypes.c_uint32(chip), None, ctypes.c_uint64(0))
        if n < 0:
            raise IndexError(chip)
        out = np.zeros(n, dtype=np.uint32)
        fn(self._h, ctypes.c_uint32(chip), out.ctypes.data_as(c_u32p), ctypes.c_uint64(n))
        return out

    def debug_perm_trace(self, chip):
        return self._dbg(lib().vgpu_proof_debug_perm_trace, chip)

    def debug_quotient(self, chip):
        return self._dbg(lib().vgpu_proof_debug_quotient, chip)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_proof_free(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None


CBOR_CANONICAL_FIELDS, CBOR_PLAIN_DIGESTS = 1, 2


def proof_cbor(words, flags=0):
    """CBOR bytes of a proof given as VPF1 words (ciborium image of MachineProof; host-only, no device needed)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    L = lib()
    L.vgpu_proof_cbor.restype = ctypes.c_int64
    n = L.vgpu_proof_cbor(w.ctypes.data_as(c_u32p), ctypes.c_uint64(w.size), ctypes.c_uint32(flags), None, ctypes.c_uint64(0))
    if n < 0:
        _check(int(n))
    buf = (ctypes.c_uint8 * int(n))()
    L.vgpu_proof_cbor(w.ctypes.data_as(c_u32p), ctypes.c_uint64(w.size), ctypes.c_uint32(flags), buf, ctypes.c_uint64(int(n)))
    return bytes(buf)


def proof_from_cbor(data):
    """VPF1 proof words from the CBOR image of a MachineProof (vgpu_proof_from_cbor: what `ciborium::from_reader` does on the verifier's
    side; host-only).  Either setting of the two encoding switches is accepted.  Raises VgpuError on malformed input."""
    b = bytes(data)
    buf = (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    L = lib()
    L.vgpu_proof_from_cbor.restype = ctypes.c_int64
    n = L.vgpu_proof_from_cbor(buf, ctypes.c_uint64(len(b)), None, ctypes.c_uint64(0))
    if n < 0:
        _check(int(n))
    out = np.zeros(int(n), dtype=np.uint32)
    L.vgpu_proof_from_cbor(buf, ctypes.c_uint64(len(b)), out.ctypes.data_as(c_u32p), ctypes.c_uint64(int(n)))
    return out


def proof_from_cbor_ex(data, bare_is_montgomery=False):
    """(proof words, forms seen) — vgpu_proof_from_cbor_ex: the decoder with the one reading the image itself cannot decide (a bare integer as
    the Montgomery word) selectable, and a report of the encodings met: bit 1 field as {"value": m}, 2 field bare, 4 digest as Hash struct, 8 plain."""
    b = bytes(data)
    buf = (ctypes.c_uint8 * max(1, len(b))).from_buffer_copy(b if b else b"\0")
    L = lib()
    L.vgpu_proof_from_cbor_ex.restype = ctypes.c_int64
    seen = ctypes.c_uint32(0)
    fl = ctypes.c_uint32(1 if bare_is_montgomery else 0)
    n = L.vgpu_proof_from_cbor_ex(buf, ctypes.c_uint64(len(b)), fl, None, ctypes.c_uint64(0), ctypes.byref(seen))
    if n < 0:
        _check(int(n))
    out = np.zeros(int(n), dtype=np.uint32)
    L.vgpu_proof_from_cbor_ex(buf, ctypes.c_uint64(len(b)), fl, out.ctypes.data_as(c_u32p), ctypes.c_uint64(int(n)), ctypes.byref(seen))
    return out, int(seen.value)


class Comm:
    """RCCL communicator owned by the library (one process per GPU): the path's one collective without Python in the loop."""

    def __init__(self, prover, unique_id, rank, world):
        self._prover, self.rank, self.world = prover, rank, world
        self._h = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(unique_id))
        _check(lib().vgpu_comm_init(prover._h, buf, ctypes.c_uint32(rank), ctypes.c_uint32(world), ctypes.byref(self._h)))

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check(lib().vgpu_comm_unique_id(buf))
        return bytes(buf)

    def set_timeout_ms(self, timeout_ms):
        """Deadline of every collective of this communicator (vgpu_comm_set_timeout_ms): past it the communicator is aborted and the call fails."""
        _check(lib().vgpu_comm_set_timeout_ms(self._h, ctypes.c_uint32(int(timeout_ms))))

    def commit_batches_sharded(self, traces, coset_shifts=None):
        """This rank's share of a sharded pcs.commit_batches over RCCL; returns the (common) root."""
        arr = (ctypes.c_void_p * len(traces))(*[t._h for t in traces])
        root = np.zeros(8, dtype=np.uint32)
        sh = None
        if coset_shifts is not None:
            shv, sh = _u32(coset_shifts)
        _check(lib().vgpu_commit_batches_sharded(self._prover._h, self._h, arr, ctypes.c_uint32(len(traces)), sh, root.ctypes.data_as(c_u32p)))
        return root

    def prove_sharded(self, main, preprocessed, log_min_sharded=12):
        """This rank's share of ONE proof sharded over the communicator's ranks (vgpu_prove_sharded); every rank passes the same traces
        (uploaded through its own prover) and receives the proof vgpu_prove gives on one GPU."""
        arr = (ctypes.c_void_p * len(main))(*[t._h for t in main])
        chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
        parr = (ctypes.c_void_p * max(1, len(preprocessed)))(*[t._h for _, t in preprocessed])
        h = ctypes.c_void_p()
        _check(lib().vgpu_prove_sharded(self._prover._h, self._h, arr, ctypes.c_uint32(len(main)), chips, parr, ctypes.c_uint32(len(preprocessed)),
                                        ctypes.c_uint32(log_min_sharded), ctypes.byref(h)))
        return Proof(h)

    def allgather_roots(self, words):
        w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
        out = np.zeros(w.size * self.world, dtype=np.uint32)
        _check(lib().vgpu_comm_allgather_roots(self._h, w.ctypes.data_as(c_u32p), ctypes.c_uint32(w.size), out.ctypes.data_as(c_u32p)))
        return out.reshape(self.world, w.size)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_comm_destroy(self._h)
            except TypeError:  # interpreter shutdown
                pass
            self._h = None


def verify_multi_batches(commits, heights, widths, points, values, proof_words, challenger, rc, log_blowup=1, num_queries=40, pow_bits=8,
                         hash_kind=HASH_KECCAK256, observe_final_poly=False):
    """pcs.verify_multi_batches on the host (vgpu_verify_multi_batches): commits[r] = 8 words; heights[r][i], widths[r][i] =
    Dimensions of matrix i of round r; points[r][i] = list of Ext5; values = flat words as open_multi_batches returned them (or the
    nested (width, 5) arrays).  Returns None if accepted, else the rejection message."""
    cfg = VgpuConfig()
    cfg.log_blowup, cfg.num_queries, cfg.pow_bits, cfg.hash_kind, cfg.observe_final_poly = log_blowup, num_queries, pow_bits, int(hash_kind), int(observe_final_poly)
    r = np.ascontiguousarray(rc, dtype=np.uint32)
    ctypes.memmove(cfg.poseidon_rc, r.ctypes.data, 480 * 4)
    c, cp = _u32(np.concatenate([np.asarray(x, dtype=np.uint32) for x in commits]))
    nm = np.array([len(h) for h in heights], dtype=np.uint32)
    hs = np.array([h for rnd in heights for h in rnd], dtype=np.uint64)
    ws = np.array([w for rnd in widths for w in rnd], dtype=np.uint32)
    npts = np.array([len(p) for rnd in points for p in rnd], dtype=np.uint32)
    pts = np.array([w for rnd in points for p in rnd for z in p for w in z], dtype=np.uint32)
    if isinstance(values, (list, tuple)):
        values = np.concatenate([v.ravel() for rnd in values for mat in rnd for v in mat])
    v, vp = _u32(values)
    pw, pwp = _u32(proof_words)
    code = lib().vgpu_verify_multi_batches(ctypes.byref(cfg), cp, ctypes.c_uint32(len(commits)), nm.ctypes.data_as(c_u32p), hs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                                           ws.ctypes.data_as(c_u32p), npts.ctypes.data_as(c_u32p), pts.ctypes.data_as(c_u32p), vp, ctypes.c_uint64(v.size), pwp,
                                           ctypes.c_uint64(pw.size), challenger._h)
    return None if code == 0 else lib().vgpu_last_error().decode()


def _config(rc, log_blowup=1, num_queries=40, pow_bits=8, hash_kind=HASH_KECCAK256, observe_final_poly=False):
    cfg = VgpuConfig()
    cfg.log_blowup, cfg.num_queries, cfg.pow_bits, cfg.hash_kind, cfg.observe_final_poly = log_blowup, num_queries, pow_bits, int(hash_kind), int(observe_final_poly)
    r = np.ascontiguousarray(rc, dtype=np.uint32)
    ctypes.memmove(cfg.poseidon_rc, r.ctypes.data, 480 * 4)
    return cfg


def verify(machine, rc, proof_words, preprocessed_commit=None, **cfg_kw):
    """Machine::verify on the host (vgpu_verify; no device needed): None if the proof is accepted, else the rejection message.
    preprocessed_commit: 8 words (host_commit_root of the preprocessed traces, as the reference's verifier recomputes it), None for a machine without."""
    cfg = _config(rc, **cfg_kw)
    pw, pwp = _u32(proof_words)
    pc = None
    if preprocessed_commit is not None:
        pcv, pc = _u32(preprocessed_commit)
    code = lib().vgpu_verify(ctypes.byref(cfg), machine._h, pc, pwp, ctypes.c_uint64(pw.size))
    return None if code == 0 else lib().vgpu_last_error().decode()


class Verifier:
    """Machine::verify of many proofs at once on one MI355X (vgpu_verify_batch): every Merkle opening, reduced opening and FRI fold on the
    device, the transcript, shapes and out-of-domain constraints on at most 16 host threads.  Same verdicts and messages as verify()."""

    def __init__(self, machine, rc, device=0, **cfg_kw):
        cfg = _config(rc, **cfg_kw)
        cfg.device = device
        self.machine = machine  # keeps the handle alive (the description is copied, but a caller may expect the pair)
        self._h = ctypes.c_void_p()
        _check(lib().vgpu_verifier_create(ctypes.byref(cfg), machine._h, ctypes.byref(self._h)))

    def set_chunk_words(self, words):
        """Proof words per device chunk (default 2^25): a batch is checked in chunks of at most this many words."""
        _check(lib().vgpu_verifier_set_chunk_words(self._h, ctypes.c_uint64(int(words))))

    def set_poison(self, word=None):
        """Test hook (vgpu_verifier_set_poison): with a word, every chunk first fills the verifier's whole reused device buffer with it; None = off."""
        _check(lib().vgpu_verifier_set_poison(self._h, ctypes.c_uint32(0 if word is None else 1), ctypes.c_uint32(0 if word is None else int(word))))

    def verify_batch(self, proofs, preprocessed_commits=None):
        """proofs: list of word arrays; preprocessed_commits: one 8-word array per proof, or None for a machine without preprocessed traces.
        Returns one entry per proof: None if accepted, else the rejection message (as verify())."""
        n = len(proofs)
        keep = [np.ascontiguousarray(p, dtype=np.uint32) for p in proofs]
        ptrs = (c_u32p * max(n, 1))(*[k.ctypes.data_as(c_u32p) for k in keep])
        nw = (ctypes.c_uint64 * max(n, 1))(*[k.size for k in keep])
        pc = None
        if preprocessed_commits is not None:
            assert len(preprocessed_commits) == n
            pcv, pc = _u32(np.concatenate([np.asarray(c, dtype=np.uint32).ravel() for c in preprocessed_commits]) if n else np.zeros(8, np.uint32))
        status = (ctypes.c_int32 * max(n, 1))()
        _check(lib().vgpu_verify_batch(self._h, ptrs, nw, pc, ctypes.c_uint32(n), status))
        out = []
        for i in range(n):
            if status[i] == 0:
                out.append(None)
                continue
            m = int(lib().vgpu_verifier_message(self._h, ctypes.c_uint32(i), None, ctypes.c_uint64(0)))
            buf = ctypes.create_string_buffer(m + 1)
            lib().vgpu_verifier_message(self._h, ctypes.c_uint32(i), buf, ctypes.c_uint64(m + 1))
            out.append(buf.value.decode())
        return out

    def timing(self):
        """(host ms, device ms) of the last verify_batch call."""
        h, d = ctypes.c_double(), ctypes.c_double()
        lib().vgpu_verifier_timing(self._h, ctypes.byref(h), ctypes.byref(d))
        return h.value, d.value

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_verifier_destroy(self._h)
            except TypeError:  # interpreter shutdown
                pass
            self._h = None


def host_commit_root(matrices, rc, coset_shifts=None, **cfg_kw):
    """pcs.commit_batches on the host (vgpu_host_commit_root): the root vgpu_commit_batches gives on the device; for the small matrices a
    verifier commits itself."""
    cfg = _config(rc, **cfg_kw)
    keep = [np.ascontiguousarray(m, dtype=np.uint32) for m in matrices]
    ptrs = (c_u32p * len(keep))(*[k.ctypes.data_as(c_u32p) for k in keep])
    hs = (ctypes.c_uint64 * len(keep))(*[k.shape[0] for k in keep])
    ws = (ctypes.c_uint64 * len(keep))(*[k.shape[1] for k in keep])
    sh = None
    if coset_shifts is not None:
        shv, sh = _u32(coset_shifts)
    root = np.zeros(8, dtype=np.uint32)
    _check(lib().vgpu_host_commit_root(ctypes.byref(cfg), ptrs, hs, ws, ctypes.c_uint32(len(keep)), sh, root.ctypes.data_as(c_u32p)))
    return root


def commit_batches_sharded_local(provers, matrices, coset_shifts=None):
    """One commitment round sharded over len(provers) prover contexts of this process (vgpu_commit_batches_sharded_local):
    returns the root, which equals provers[0].commit_batches(..).root."""
    keep = [[p.upload(m) for m in matrices] for p in provers]
    arr = (ctypes.c_void_p * (len(provers) * len(matrices)))(*[t._h for row in keep for t in row])
    parr = (ctypes.c_void_p * len(provers))(*[p._h for p in provers])
    root = np.zeros(8, dtype=np.uint32)
    sh = None
    if coset_shifts is not None:
        shv, sh = _u32(coset_shifts)
    _check(lib().vgpu_commit_batches_sharded_local(parr, ctypes.c_uint32(len(provers)), arr, ctypes.c_uint32(len(matrices)), sh, root.ctypes.data_as(c_u32p)))
    return root


def upload_replicated(provers, main_traces, preprocessed):
    """The traces of one proof uploaded through every prover context (a sharded proof replicates the traces): (main, prep) handles for
    prove_sharded_local(.., uploaded=..)."""
    return [[p.upload(m) for m in main_traces] for p in provers], [[p.upload(m) for _, m in preprocessed] for p in provers]


def sharded_trace_is_split(world, height, log_blowup=1, log_min_sharded=12):
    """vgpu_sharded_trace_is_split: whether a chip of this trace height hands in row ranges (its LDE is sharded) in the row-range form of a sharded proof."""
    f = lib().vgpu_sharded_trace_is_split
    f.restype = ctypes.c_uint32
    return bool(f(ctypes.c_uint32(world), ctypes.c_uint32(log_blowup), ctypes.c_uint32(log_min_sharded), ctypes.c_uint64(int(height))))


def row_ranges(main_traces, rank, world, log_blowup=1, log_min_sharded=12):
    """Rank `rank`'s inputs of a sharded proof in ROW-RANGE form: (matrices, full_heights) — the rows [rank n / world, (rank + 1) n / world) of every chip
    whose LDE is sharded, the whole trace of every other chip."""
    out, full = [], []
    for m in main_traces:
        n = m.shape[0]
        full.append(n)
        if sharded_trace_is_split(world, n, log_blowup, log_min_sharded):
            out.append(np.ascontiguousarray(m[rank * (n // world):(rank + 1) * (n // world)]))
        else:
            out.append(m)
    return out, full


def upload_row_ranges(provers, main_traces, preprocessed, log_min_sharded=12):
    """The ROW-RANGE inputs of one sharded proof uploaded through the prover contexts standing in for the ranks: context r gets only its rows of
    every sharded chip.  For prove_sharded_rows_local(.., uploaded=..)."""
    keep, full = [], None
    for r, p in enumerate(provers):
        mats, full = row_ranges(main_traces, r, len(provers), p.log_blowup, log_min_sharded)
        keep.append([p.upload(m) for m in mats])
    return keep, [[p.upload(m) for _, m in preprocessed] for p in provers], full


def prove_sharded_rows_local(provers, main_traces, preprocessed, log_min_sharded=12, uploaded=None):
    """ONE proof over len(provers) prover contexts of this process with the TRACES sharded too (vgpu_prove_sharded_rows_local): context r uploads only
    its row range of every sharded chip (row_ranges).  Returns the Proof, word for word provers[0].prove(..) of the whole traces."""
    W = len(provers)
    keep, keep_p, full = uploaded if uploaded is not None else upload_row_ranges(provers, main_traces, preprocessed, log_min_sharded)
    arr = (ctypes.c_void_p * (W * len(main_traces)))(*[t._h for row in keep for t in row])
    fh = (ctypes.c_uint64 * len(main_traces))(*full)
    chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
    parr = (ctypes.c_void_p * max(1, W * len(preprocessed)))(*[t._h for row in keep_p for t in row])
    pv = (ctypes.c_void_p * W)(*[p._h for p in provers])
    h = ctypes.c_void_p()
    _check(lib().vgpu_prove_sharded_rows_local(pv, ctypes.c_uint32(W), arr, ctypes.c_uint32(len(main_traces)), fh, chips, parr, ctypes.c_uint32(len(preprocessed)),
                                               ctypes.c_uint32(log_min_sharded), ctypes.byref(h)))
    return Proof(h)


class VgpuFabric(ctypes.Structure):
    """vgpu_fabric_t (include/vgpu.h): the host's own transport for a sharded proof, two collective callbacks over host buffers."""
    ALL_GATHER = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, c_u32p, ctypes.c_uint64, c_u32p)
    ALL_TO_ALL = ctypes.CFUNCTYPE(ctypes.c_int32, ctypes.c_void_p, ctypes.POINTER(c_u32p), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(c_u32p),
                                  ctypes.POINTER(ctypes.c_uint64))
    _fields_ = [("struct_size", ctypes.c_uint32), ("timeout_ms", ctypes.c_uint32), ("user", ctypes.c_void_p), ("rank", ctypes.c_uint32), ("world", ctypes.c_uint32),
                ("all_gather", ALL_GATHER), ("all_to_all", ALL_TO_ALL)]


_ABANDONED_FABRICS = []  # fabrics whose callbacks the library gave up on at its deadline: a helper thread of the library may still be INSIDE one of their ctypes thunks, so they live as long as the process


class Fabric:
    """A caller-supplied fabric from two Python callables (what a Rust host would write against its own transport):
        all_gather(mine: np.uint32[n]) -> np.uint32[world, n]
        all_to_all(send: list of np.uint32 arrays or None per rank, recv_words: list of int) -> list of np.uint32 arrays (None where 0 words)
    Exceptions inside a callback become a non-zero status: the proof is abandoned on every rank (the library's failure protocol).
    timeout_ms > 0: the library bounds every callback (vgpu_fabric_t::timeout_ms) — it then calls them from a helper thread of its own."""

    def __init__(self, rank, world, all_gather, all_to_all, timeout_ms=0):
        self.rank, self.world = rank, world
        self.errors = []
        self._ag_py, self._a2a_py = all_gather, all_to_all  # looked up at call time: a test may wrap them

        def ag(_user, words, n, out):
            try:
                mine = np.ctypeslib.as_array(words, shape=(int(n),)).copy()
                got = np.ascontiguousarray(self._ag_py(mine), dtype=np.uint32).reshape(world, int(n))
                ctypes.memmove(out, got.ctypes.data, got.nbytes)
                return 0
            except Exception as e:  # noqa: BLE001 - must not unwind into C
                self.errors.append(e)
                return 1

        def a2a(_user, send, send_words, recv, recv_words):
            try:
                sb = [np.ctypeslib.as_array(send[s], shape=(int(send_words[s]),)).copy() if send_words[s] else None for s in range(world)]
                rw = [int(recv_words[s]) for s in range(world)]
                got = self._a2a_py(sb, rw)
                for s in range(world):
                    if rw[s]:
                        g = np.ascontiguousarray(got[s], dtype=np.uint32).reshape(-1)
                        assert g.size == rw[s], "all_to_all delivered %d words from rank %d, expected %d" % (g.size, s, rw[s])
                        ctypes.memmove(recv[s], g.ctypes.data, g.nbytes)
                return 0
            except Exception as e:  # noqa: BLE001
                self.errors.append(e)
                return 1

        self._ag, self._a2a = VgpuFabric.ALL_GATHER(ag), VgpuFabric.ALL_TO_ALL(a2a)  # kept alive with the object
        self.c = VgpuFabric(ctypes.sizeof(VgpuFabric), int(timeout_ms), None, rank, world, self._ag, self._a2a)

    @staticmethod
    def over_torch_distributed(dist, group=None, timeout_ms=0):
        """The exchanges through a torch.distributed process group on CPU tensors (gloo): all_gather, and pairwise isend / irecv."""
        import torch

        rank, world = dist.get_rank(group), dist.get_world_size(group)

        def all_gather(mine):
            outs = [torch.zeros(mine.size, dtype=torch.int32) for _ in range(world)]
            dist.all_gather(outs, torch.from_numpy(mine.view(np.int32).copy()), group=group)
            return np.stack([o.numpy().view(np.uint32) for o in outs])

        def all_to_all(send, recv_words):
            reqs, bufs = [], [None] * world
            for s in range(world):
                if s != rank and recv_words[s]:
                    bufs[s] = torch.zeros(recv_words[s], dtype=torch.int32)
                    reqs.append(dist.irecv(bufs[s], src=s, group=group))
            keep = []
            for s in range(world):
                if s != rank and send[s] is not None:
                    t = torch.from_numpy(send[s].view(np.int32))
                    keep.append(t)
                    reqs.append(dist.isend(t, dst=s, group=group))
            for r in reqs:
                r.wait()
            return [None if b is None else b.numpy().view(np.uint32) for b in bufs]

        return Fabric(rank, world, all_gather, all_to_all, timeout_ms=timeout_ms)

    def selftest(self, n_words=17, fail_rank=0xFFFFFFFF):
        """vgpu_fabric_selftest: None if this rank's exchanges were all correct, else the library's message (a failing peer included)."""
        code = lib().vgpu_fabric_selftest(ctypes.byref(self.c), ctypes.c_uint32(n_words), ctypes.c_uint32(fail_rank))
        return None if code == 0 else lib().vgpu_last_error().decode()

    def prove_sharded(self, prover, main, preprocessed, log_min_sharded=12, full_heights=None):
        """This rank's share of ONE proof sharded over the fabric's ranks (vgpu_prove_sharded_fabric): every rank passes the same traces,
        uploaded through its own prover, and receives the proof vgpu_prove gives on one GPU.  full_heights given: the ROW-RANGE form
        (vgpu_prove_sharded_rows_fabric) — `main` holds this rank's rows of every sharded chip (row_ranges)."""
        arr = (ctypes.c_void_p * len(main))(*[t._h for t in main])
        chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
        parr = (ctypes.c_void_p * max(1, len(preprocessed)))(*[t._h for _, t in preprocessed])
        h = ctypes.c_void_p()
        try:
            if full_heights is not None:
                fh = (ctypes.c_uint64 * len(main))(*[int(x) for x in full_heights])
                _check(lib().vgpu_prove_sharded_rows_fabric(prover._h, ctypes.byref(self.c), arr, ctypes.c_uint32(len(main)), fh, chips, parr, ctypes.c_uint32(len(preprocessed)),
                                                            ctypes.c_uint32(log_min_sharded), ctypes.byref(h)))
                return Proof(h)
            _check(lib().vgpu_prove_sharded_fabric(prover._h, ctypes.byref(self.c), arr, ctypes.c_uint32(len(main)), chips, parr, ctypes.c_uint32(len(preprocessed)),
                                                   ctypes.c_uint32(log_min_sharded), ctypes.byref(h)))
            return Proof(h)
        except VgpuError as e:
            # only a callback ABANDONED at the deadline (VGPU_ERR_FABRIC with the library's "callback is abandoned", csrc/host/fabric.hpp) leaves a library
            # thread inside one of this object's thunks: those must stay valid for the life of the process.  Argument errors, dead peers and failpoints
            # leave nothing behind, and a host that retries must not pin every Fabric it ever made.
            if self.c.timeout_ms and e.code == -6 and "callback is abandoned" in str(e) and not any(f is self for f in _ABANDONED_FABRICS):
                _ABANDONED_FABRICS.append(self)
            raise


def prove_sharded_local(provers, main_traces, preprocessed, log_min_sharded=12, uploaded=None):
    """ONE proof over len(provers) prover contexts of this process standing in for the ranks (vgpu_prove_sharded_local): main_traces are
    host matrices (chip order), preprocessed a list of (chip, host matrix); every context gets its own upload (the traces are replicated,
    the LDEs / trees / FRI layers are sharded) unless `uploaded` = upload_replicated(..) hands them in.  Returns the Proof, word for word
    provers[0].prove(..) of the same traces."""
    keep_m, keep_p = uploaded if uploaded is not None else upload_replicated(provers, main_traces, preprocessed)
    arr = (ctypes.c_void_p * (len(provers) * len(main_traces)))(*[t._h for row in keep_m for t in row])
    chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
    parr = (ctypes.c_void_p * max(1, len(provers) * len(preprocessed)))(*[t._h for row in keep_p for t in row])
    pv = (ctypes.c_void_p * len(provers))(*[p._h for p in provers])
    h = ctypes.c_void_p()
    _check(lib().vgpu_prove_sharded_local(pv, ctypes.c_uint32(len(provers)), arr, ctypes.c_uint32(len(main_traces)), chips, parr, ctypes.c_uint32(len(preprocessed)),
                                          ctypes.c_uint32(log_min_sharded), ctypes.byref(h)))
    return Proof(h)


# ---- the witness audits.  Each has its options, its report class and its public functions below; what they share is here.
class _AuditReport:
    def to_json(self):
        import json

        return json.dumps(self.to_dict())


def _chip_mask(name, chips):
    """chips (None: every chip) as the chip_mask of the options of `name`_audit; refused here, with the library's status code."""
    mask = 0
    if chips is not None:
        cs = [int(c) for c in chips]
        if not cs or any(c < 0 or c > 31 for c in cs):
            raise VgpuError(-1, "%s_audit: chips is a non-empty list of chip indices below 32" % name)
        for c in cs:
            mask |= 1 << c
    return mask


def _audit_report(name, cls, h):
    """The handle h of a vgpu_`name`_report_t as a `cls`, and the handle freed."""
    L = lib()
    length, words_of, timing, free = (getattr(L, "vgpu_%s_report_%s" % (name, f)) for f in ("len", "words", "timing", "free"))
    length.restype = ctypes.c_uint64
    words_of.restype = c_u32p
    length.argtypes = words_of.argtypes = free.argtypes = [ctypes.c_void_p]
    timing.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    try:
        words = np.ctypeslib.as_array(words_of(h), shape=(int(length(h)),)).copy()
        tm = (ctypes.c_double * (2 if name in ("bus", "constraint") else 3))()  # device_ms, host_ms and, but for these two, evaluations
        timing(h, tm)
    finally:
        free(h)
    return cls(words, *tm)


def _audit_host(name, machine, main_matrices, preprocessed, opts):
    """vgpu_`name`_audit_host: main_matrices = one canonical matrix per chip, preprocessed = [(chip index, matrix)], opts = the audit's options."""
    mains = [np.ascontiguousarray(m, dtype=np.uint32) for m in main_matrices]
    preps = [(int(c), np.ascontiguousarray(m, dtype=np.uint32)) for c, m in preprocessed]
    for m in mains + [m for _, m in preps]:
        if m.ndim != 2:
            raise VgpuError(-1, "%s_audit: traces are two-dimensional matrices" % name)

    def arrays(ms):
        n = max(1, len(ms))
        return ((ctypes.c_void_p * n)(*[m.ctypes.data for m in ms]), (ctypes.c_uint64 * n)(*[m.shape[0] for m in ms]), (ctypes.c_uint64 * n)(*[m.shape[1] for m in ms]))

    mp, mh, mw = arrays(mains)
    pp, ph, pw = arrays([m for _, m in preps])
    chips = (ctypes.c_uint32 * max(1, len(preps)))(*[c for c, _ in preps])
    h = ctypes.c_void_p()
    _check(getattr(lib(), "vgpu_%s_audit_host" % name)(machine._h, mp, mh, mw, ctypes.c_uint32(len(mains)), chips, pp, ph, pw, ctypes.c_uint32(len(preps)), ctypes.byref(opts),
                                                        ctypes.byref(h)))
    return _audit_report(name, _AUDIT_REPORTS[name], h)


class BusAuditOpts(ctypes.Structure):  # vgpu_bus_audit_opts_t
    _fields_ = [("max_tuples", ctypes.c_uint64), ("max_records_per_tuple", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32)]


BUS_NAMES = {(1, 0): "general", (1, 1): "program", (1, 2): "memory", (1, 3): "range"}  # BasicMachine's global buses (basic/src/lib.rs: bus indices)


class BusReport:
    """The bus audit of a witness (vgpu_bus_audit / vgpu_bus_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    balanced, truncated, total_unbalanced, reported, buses = [dict(bus=(is_global, bus_index), width, live, sends, receives, unbalanced)],
    tuples = [dict(bus, fields, net, net_signed, send_sum, recv_sum, n_send, n_recv, records=[(chip, row, interaction, is_send, count)])],
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call)."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31524256 or w[1] != len(w):
            raise ValueError("not a bus report image")
        self.words = np.array(w, dtype=np.uint32)
        self.balanced, self.truncated = bool(w[2]), bool(w[3])
        self.total_unbalanced, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms = float(device_ms), float(host_ms)
        pos = 8
        self.buses = []
        for _ in range(w[7]):
            live, sends, recvs, unb = (w[pos + 4 + 2 * k] | (w[pos + 5 + 2 * k] << 32) for k in range(4))
            self.buses.append(dict(bus=(w[pos], w[pos + 1]), width=w[pos + 2], live=live, sends=sends, receives=recvs, unbalanced=unb))
            pos += 12
        self.tuples = []
        for _ in range(self.reported):
            width, net, n_listed = w[pos + 2], w[pos + 3], w[pos + 10]
            t = dict(bus=(w[pos], w[pos + 1]), net=net, net_signed=net if net <= P // 2 else net - P, send_sum=w[pos + 4], recv_sum=w[pos + 5],
                     n_send=w[pos + 6] | (w[pos + 7] << 32), n_recv=w[pos + 8] | (w[pos + 9] << 32), fields=w[pos + 11:pos + 11 + width])
            pos += 11 + width
            t["records"] = [tuple(w[pos + 5 * k:pos + 5 * k + 5]) for k in range(n_listed)]
            pos += 5 * n_listed
            self.tuples.append(t)
        assert pos == len(w)

    def to_json(self):
        import json

        return json.dumps(dict(balanced=self.balanced, truncated=self.truncated, total_unbalanced=self.total_unbalanced, reported=self.reported,
                               device_ms=self.device_ms, host_ms=self.host_ms, buses=[dict(b, bus=list(b["bus"])) for b in self.buses],
                               tuples=[dict(t, bus=list(t["bus"]), records=[list(r) for r in t["records"]]) for t in self.tuples]))


def _bus_opts(max_tuples, max_records_per_tuple, hash_bits):
    # in the C struct a zero field selects its default, so the refusals of explicit zeros are made here, with the library's status code
    if not 1 <= int(hash_bits) <= 64:
        raise VgpuError(-1, "bus_audit: hash_bits must be 1..64")
    if int(max_tuples) < 1 or int(max_records_per_tuple) < 1:
        raise VgpuError(-1, "bus_audit: max_tuples and max_records_per_tuple must be at least 1")
    return BusAuditOpts(int(max_tuples), int(max_records_per_tuple), int(hash_bits))


def bus_audit_host(machine, main_matrices, preprocessed, max_tuples=64, max_records_per_tuple=4, hash_bits=64):
    """The bus audit on the HOST (vgpu_bus_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)].  hash_bits is accepted for symmetry with Prover.bus_audit (the host groups by full tuples)."""
    opts = _bus_opts(max_tuples, max_records_per_tuple, hash_bits)
    return _audit_host("bus", machine, main_matrices, preprocessed, opts)


class ConstraintAuditOpts(ctypes.Structure):  # vgpu_constraint_audit_opts_t
    _fields_ = [("max_constraints", ctypes.c_uint64), ("max_rows_per_constraint", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class ConstraintReport(_AuditReport):
    """The constraint audit of a witness (vgpu_constraint_audit / vgpu_constraint_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: satisfied, truncated, total_failing (failing (chip, constraint) pairs), reported,
    chips = [dict(chip, constraints, failing_constraints, height, failing_rows)], constraints = [dict(chip, constraint, failing_rows,
    rows=[(row, value)])] ascending by (chip, constraint), device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call)."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31524356 or w[1] != len(w):
            raise ValueError("not a constraint report image")
        self.words = np.array(w, dtype=np.uint32)
        self.satisfied, self.truncated = bool(w[2]), bool(w[3])
        self.total_failing, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms = float(device_ms), float(host_ms)
        pos = 8
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, constraints=w[pos], failing_constraints=w[pos + 1], height=w[pos + 2] | (w[pos + 3] << 32), failing_rows=w[pos + 4] | (w[pos + 5] << 32)))
            pos += 6
        self.constraints = []
        for _ in range(self.reported):
            n_listed = w[pos + 4]
            e = dict(chip=w[pos], constraint=w[pos + 1], failing_rows=w[pos + 2] | (w[pos + 3] << 32))
            pos += 5
            e["rows"] = [(w[pos + 2 * k], w[pos + 2 * k + 1]) for k in range(n_listed)]
            pos += 2 * n_listed
            self.constraints.append(e)
        assert pos == len(w)

    def to_dict(self):
        return dict(satisfied=self.satisfied, truncated=self.truncated, total_failing=self.total_failing, reported=self.reported, device_ms=self.device_ms,
                    host_ms=self.host_ms, chips=self.chips, constraints=[dict(e, rows=[list(r) for r in e["rows"]]) for e in self.constraints])


def _constraint_opts(max_constraints, max_rows_per_constraint):
    # in the C struct a zero field selects its default, so the refusals of explicit zeros are made here, with the library's status code
    if int(max_constraints) < 1 or int(max_rows_per_constraint) < 1:
        raise VgpuError(-1, "constraint_audit: max_constraints and max_rows_per_constraint must be at least 1")
    return ConstraintAuditOpts(int(max_constraints), int(max_rows_per_constraint), 0)


def constraint_audit_host(machine, main_matrices, preprocessed, max_constraints=64, max_rows_per_constraint=4):
    """The constraint audit on the HOST (vgpu_constraint_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)]; a ConstraintReport back."""
    opts = _constraint_opts(max_constraints, max_rows_per_constraint)
    return _audit_host("constraint", machine, main_matrices, preprocessed, opts)


class MutationAuditOpts(ctypes.Structure):  # vgpu_mutation_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("n_deltas", ctypes.c_uint32), ("deltas", ctypes.c_uint32 * 4),
                ("reserved", ctypes.c_uint32 * 2)]


class MutationReport(_AuditReport):
    """The mutation audit of a witness (vgpu_mutation_audit / vgpu_mutation_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: deltas, truncated, total_entries ((chip, column, delta) with a free row), reported,
    chips = [dict(chip, width, constraints, height, unbound, free=[per delta], air=[..], bus=[..])] (sums over the chip's columns),
    entries = [dict(chip, column, delta, free, air, bus, rows=[first free rows])] ascending by (chip, column, delta index; `delta` is the index),
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (Air::eval row evaluations performed)."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 12 or w[0] != 0x31524D56 or w[1] != len(w) or not 1 <= w[2] <= 4:
            raise ValueError("not a mutation report image")
        self.words = np.array(w, dtype=np.uint32)
        D = w[2]
        self.deltas, self.truncated = w[8:8 + D], bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 12
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], height=u64(pos + 2), unbound=w[pos + 4], free=[u64(pos + 6 + 6 * i) for i in range(D)],
                                   air=[u64(pos + 8 + 6 * i) for i in range(D)], bus=[u64(pos + 10 + 6 * i) for i in range(D)]))
            pos += 6 + 6 * D
        self.entries = []
        for _ in range(self.reported):
            n_listed = w[pos + 3]
            e = dict(chip=w[pos], column=w[pos + 1], delta=w[pos + 2], free=u64(pos + 4), air=u64(pos + 6), bus=u64(pos + 8), rows=w[pos + 10:pos + 10 + n_listed])
            pos += 10 + n_listed
            self.entries.append(e)
        assert pos == len(w)

    def unbound_columns(self, chip):
        """The columns of `chip` that are free on every row for every delta — as far as the list goes (exact when not truncated)."""
        height, D = self.chips[chip]["height"], len(self.deltas)
        full = {}
        for e in self.entries:
            if e["chip"] == chip and e["free"] == height:
                full[e["column"]] = full.get(e["column"], 0) + 1
        return sorted(c for c, k in full.items() if k == D)

    def to_dict(self):
        return dict(deltas=self.deltas, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _mutation_opts(deltas, max_entries, max_rows_per_entry):
    # in the C struct a zero field selects its default, so the refusals of explicit zeros (and of an empty delta list) are made here, with the
    # library's status code; the range and distinctness of the deltas are the library's to check
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1:
        raise VgpuError(-1, "mutation_audit: max_entries and max_rows_per_entry must be at least 1")
    ds = [int(d) for d in ((1, P - 1) if deltas is None else deltas)]
    if not 1 <= len(ds) <= 4:
        raise VgpuError(-1, "mutation_audit: 1 to 4 deltas (got %d)" % len(ds))
    if any(d < 0 or d > 0xFFFFFFFF for d in ds):
        raise VgpuError(-1, "mutation_audit: a delta must be a canonical value in 1..p-1")
    return MutationAuditOpts(int(max_entries), int(max_rows_per_entry), len(ds), (ctypes.c_uint32 * 4)(*ds), (ctypes.c_uint32 * 2)(0, 0))


def mutation_audit_host(machine, main_matrices, preprocessed, deltas=None, max_entries=1024, max_rows_per_entry=4):
    """The mutation audit on the HOST (vgpu_mutation_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], deltas = 1 to 4 distinct values in 1..p-1 (default (1, p - 1)); a MutationReport back."""
    opts = _mutation_opts(deltas, max_entries, max_rows_per_entry)
    return _audit_host("mutation", machine, main_matrices, preprocessed, opts)


class PairAuditOpts(ctypes.Structure):  # vgpu_pair_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("n_deltas", ctypes.c_uint32), ("deltas", ctypes.c_uint32 * 4),
                ("chip_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class PairReport(_AuditReport):
    """The pair audit of a witness (vgpu_pair_audit / vgpu_pair_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    deltas, truncated, total_entries ((chip, c1, c2, q) with a compensated row), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, coupled, slack, free=[per q], compensated=[per q])] (sums over all
    the chip's pairs; q = i * len(deltas) + j adds deltas[i] to c1 and deltas[j] to c2),
    entries = [dict(chip, c1, c2, q, free, compensated, rows=[first compensated rows])] ascending by (chip, c1, c2, q),
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (Air::eval row evaluations performed)."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 12 or w[0] != 0x31525056 or w[1] != len(w) or not 1 <= w[2] <= 4:
            raise ValueError("not a pair report image")
        self.words = np.array(w, dtype=np.uint32)
        D = w[2]
        self.deltas, self.truncated = w[8:8 + D], bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 12
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), coupled=w[pos + 6],
                                   slack=w[pos + 7], free=[u64(pos + 8 + 4 * q) for q in range(D * D)], compensated=[u64(pos + 10 + 4 * q) for q in range(D * D)]))
            pos += 8 + 4 * D * D
        self.entries = []
        for _ in range(self.reported):
            n_listed = w[pos + 4]
            self.entries.append(dict(chip=w[pos], c1=w[pos + 1], c2=w[pos + 2], q=w[pos + 3], free=u64(pos + 6), compensated=u64(pos + 8), rows=w[pos + 10:pos + 10 + n_listed]))
            pos += 10 + n_listed
        assert pos == len(w)

    def slack_pairs(self, chip):
        """The pairs (c1, c2) of `chip` with a compensated row for some delta pair — as far as the list goes (exact when not truncated)."""
        return sorted(set((e["c1"], e["c2"]) for e in self.entries if e["chip"] == chip))

    def to_dict(self):
        return dict(deltas=self.deltas, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _pair_opts(deltas, max_entries, max_rows_per_entry, chips):
    # as _mutation_opts: explicit zeros and an empty delta list are refused here, with the library's status code
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1:
        raise VgpuError(-1, "pair_audit: max_entries and max_rows_per_entry must be at least 1")
    ds = [int(d) for d in ((1, P - 1) if deltas is None else deltas)]
    if not 1 <= len(ds) <= 4:
        raise VgpuError(-1, "pair_audit: 1 to 4 deltas (got %d)" % len(ds))
    if any(d < 0 or d > 0xFFFFFFFF for d in ds):
        raise VgpuError(-1, "pair_audit: a delta must be a canonical value in 1..p-1")
    return PairAuditOpts(int(max_entries), int(max_rows_per_entry), len(ds), (ctypes.c_uint32 * 4)(*ds), _chip_mask("pair", chips), 0)


def pair_audit_host(machine, main_matrices, preprocessed, deltas=None, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The pair audit on the HOST (vgpu_pair_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)], deltas = 1 to 4 distinct values in 1..p-1 (default (1, p - 1)), chips = the chip indices to audit (default: all);
    a PairReport back."""
    opts = _pair_opts(deltas, max_entries, max_rows_per_entry, chips)
    return _audit_host("pair", machine, main_matrices, preprocessed, opts)


class RankAuditOpts(ctypes.Structure):  # vgpu_rank_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 2)]


class RankReport(_AuditReport):
    """The rank audit of a witness (vgpu_rank_audit / vgpu_rank_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    truncated, total_entries ((chip, column) with a coupled row), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, nullity, zero, coupled_rows (sums over the rows), max_nullity,
    loose_columns, pinned_columns, coupled_columns (counts), loose=[rows per column], zeros=[rows per column])],
    entries = [dict(chip, column, coupled, rows=[dict(row, n_support, terms=[(column, coefficient)])])] ascending by (chip, column),
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations of the contract).
    First order, one row, THIS witness: not a soundness proof."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31525256 or w[1] != len(w) or w[2] != 8:
            raise ValueError("not a rank report image")
        self.words = np.array(w, dtype=np.uint32)
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 8
        self.chips = []
        for c in range(w[7]):
            wd = w[pos]
            self.chips.append(dict(chip=c, width=wd, constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), nullity=u64(pos + 6),
                                   zero=u64(pos + 8), coupled_rows=u64(pos + 10), max_nullity=w[pos + 12], loose_columns=w[pos + 13], pinned_columns=w[pos + 14],
                                   coupled_columns=w[pos + 15], loose=[u64(pos + 16 + 4 * k) for k in range(wd)], zeros=[u64(pos + 18 + 4 * k) for k in range(wd)]))
            pos += 16 + 4 * wd
        self.entries = []
        for _ in range(self.reported):
            rows = []
            for k in range(w[pos + 2]):
                at = pos + 6 + 18 * k
                rows.append(dict(row=w[at], n_support=w[at + 1], terms=[(w[at + 2 + 2 * i], w[at + 3 + 2 * i]) for i in range(min(8, w[at + 1]))]))
            self.entries.append(dict(chip=w[pos], column=w[pos + 1], coupled=u64(pos + 4), rows=rows))
            pos += 6 + 18 * w[pos + 2]
        assert pos == len(w)

    def loose_columns(self, chip):
        """The columns of `chip` that are loose on some row (zero columns included)."""
        return [k for k, n in enumerate(self.chips[chip]["loose"]) if n]

    def coupled_columns(self, chip):
        """The columns of `chip` that are coupled on some row: bound alone, slack together (exact, from the per-column counts)."""
        c = self.chips[chip]
        return [k for k in range(c["width"]) if c["loose"][k] > c["zeros"][k]]

    def to_dict(self):
        return dict(truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _rank_opts(max_entries, max_rows_per_entry, chips):
    # as _pair_opts: explicit zeros are refused here, with the library's status code
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1:
        raise VgpuError(-1, "rank_audit: max_entries and max_rows_per_entry must be at least 1")
    return RankAuditOpts(int(max_entries), int(max_rows_per_entry), _chip_mask("rank", chips), (ctypes.c_uint32 * 2)(0, 0))


def rank_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The rank audit on the HOST (vgpu_rank_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)], chips = the chip indices to audit (default: all); a RankReport back."""
    opts = _rank_opts(max_entries, max_rows_per_entry, chips)
    return _audit_host("rank", machine, main_matrices, preprocessed, opts)


class StepAuditOpts(ctypes.Structure):  # vgpu_step_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("n_steps", ctypes.c_uint32),
                ("steps", ctypes.c_uint32 * 4), ("reserved", ctypes.c_uint32 * 3)]


class StepReport(_AuditReport):
    """The step audit of a witness (vgpu_step_audit / vgpu_step_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    steps (canonical), truncated, total_entries ((chip, column) with a coupled-and-exact or a curved row), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, max_degree, line_exact, loose_cells, zero_cells, exact_cells,
    coupled_exact_cells, confirmed_rows, refuted_rows, passes=[cells per step], bus, loose / zeros / exact / coupled_exact=[rows per column])],
    entries = [dict(chip, column, coupled_exact, curved, rows=[dict(row, pass_mask, zero, exact, n_support, terms=[(column, coefficient)])])]
    ascending by (chip, column), device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations.
    One row, THIS witness, the canonical null vectors only: not a soundness proof."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 14 or w[0] != 0x31525356 or w[1] != len(w) or w[2] != 8 or not 1 <= w[8] <= 4:
            raise ValueError("not a step report image")
        self.words = np.array(w, dtype=np.uint32)
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.steps = w[10:10 + w[8]]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)
        S, full = len(self.steps), (1 << len(self.steps)) - 1

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 14
        self.chips = []
        for c in range(w[7]):
            wd = w[pos]
            self.chips.append(dict(chip=c, width=wd, constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), max_degree=w[pos + 6],
                                   line_exact=bool(w[pos + 7]), loose_cells=u64(pos + 8), zero_cells=u64(pos + 10), exact_cells=u64(pos + 12), coupled_exact_cells=u64(pos + 14),
                                   confirmed_rows=u64(pos + 16), refuted_rows=u64(pos + 18), passes=[u64(pos + 20 + 2 * s) for s in range(S)], bus=u64(pos + 28),
                                   loose=[u64(pos + 30 + 8 * k) for k in range(wd)], zeros=[u64(pos + 32 + 8 * k) for k in range(wd)],
                                   exact=[u64(pos + 34 + 8 * k) for k in range(wd)], coupled_exact=[u64(pos + 36 + 8 * k) for k in range(wd)]))
            pos += 30 + 8 * wd
        self.entries = []
        for _ in range(self.reported):
            rows = []
            for k in range(w[pos + 2]):
                at = pos + 8 + 20 * k
                rows.append(dict(row=w[at], pass_mask=w[at + 1], zero=bool(w[at + 2]), exact=w[at + 1] == full, n_support=w[at + 3],
                                 terms=[(w[at + 4 + 2 * i], w[at + 5 + 2 * i]) for i in range(min(8, w[at + 3]))]))
            self.entries.append(dict(chip=w[pos], column=w[pos + 1], coupled_exact=u64(pos + 4), curved=u64(pos + 6), rows=rows))
            pos += 8 + 20 * w[pos + 2]
        assert pos == len(w)

    def confirmed_columns(self, chip):
        """The columns of `chip` that are coupled and exact on some row: a finite trade every check accepts (exact, from the per-column counts)."""
        return [k for k, n in enumerate(self.chips[chip]["coupled_exact"]) if n]

    def refuted_columns(self, chip):
        """The columns of `chip` that are curved on some row: loose to first order, caught at some step."""
        c = self.chips[chip]
        return [k for k in range(c["width"]) if c["loose"][k] > c["exact"][k]]

    def apply(self, main_traces, entry, listed_row, step):
        """A copy of the chip's trace with the move of entry['rows'][listed_row] made at step index `step`: M[r] + steps[step] v.  Only when the
        vector is listed whole (support <= 8 terms)."""
        row = entry["rows"][listed_row]
        if row["n_support"] > len(row["terms"]):
            raise VgpuError(-1, "step_audit: the vector of chip %d column %d row %d is cut (%d terms, %d listed): it cannot be applied" %
                            (entry["chip"], entry["column"], row["row"], row["n_support"], len(row["terms"])))
        t = self.steps[step]
        out = np.array(main_traces[entry["chip"]], dtype=np.uint32, copy=True)
        for col, coef in row["terms"]:
            out[row["row"], col] = (int(out[row["row"], col]) % P + t * coef) % P
        return out

    def to_dict(self):
        return dict(steps=self.steps, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _step_opts(steps, max_entries, max_rows_per_entry, chips):
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1:
        raise VgpuError(-1, "step_audit: max_entries and max_rows_per_entry must be at least 1")
    mask = _chip_mask("step", chips)
    st = [] if steps is None else [int(x) for x in steps]
    if steps is not None and not 1 <= len(st) <= 4:
        raise VgpuError(-1, "step_audit: 1 to 4 steps (got %d)" % len(st))
    if any(x < 0 or x >= 1 << 32 for x in st):
        raise VgpuError(-1, "step_audit: a step must be a canonical value in 1..p-1")
    return StepAuditOpts(int(max_entries), int(max_rows_per_entry), mask, len(st), (ctypes.c_uint32 * 4)(*st), (ctypes.c_uint32 * 3)(0, 0, 0))


def step_audit_host(machine, main_matrices, preprocessed, steps=None, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The step audit on the HOST (vgpu_step_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)], steps = 1 to 4 distinct canonical values in 1..p-1 (default 1, p - 1, 2), chips = the chip indices to audit
    (default: all); a StepReport back."""
    opts = _step_opts(steps, max_entries, max_rows_per_entry, chips)
    return _audit_host("step", machine, main_matrices, preprocessed, opts)


class InvariantAuditOpts(ctypes.Structure):  # vgpu_invariant_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("max_terms", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3)]


class InvariantReport(_AuditReport):
    """The invariant audit of a witness (vgpu_invariant_audit / vgpu_invariant_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: max_terms, truncated, total_entries (the sum of d over the audited chips), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, rank (rho_A), invariants (d), constant_columns, relations (counts),
    every, some, never (invariants enforced on every row, on some rows, on no row))],
    entries = [dict(chip, column, kind ("constant" / "relation"), l0, support, terms=[(column, coefficient)], enforced_rows, free_rows,
    rows=[the first free rows])] ascending by (chip, column): l0 + sum(coefficient * M[r][column]) = 0 on every row r of the witness,
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations of the enforcement phase).
    Affine-linear, one row, THIS witness, per basis vector, first order: candidates for missing constraints, not findings."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31524956 or w[1] != len(w):
            raise ValueError("not an invariant report image")
        self.words = np.array(w, dtype=np.uint32)
        self.max_terms = w[2]
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 8
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), rank=w[pos + 6],
                                   invariants=w[pos + 7], constant_columns=w[pos + 8], relations=w[pos + 9], every=w[pos + 10], some=w[pos + 11], never=w[pos + 12]))
            pos += 14
        self.entries = []
        for _ in range(self.reported):
            T, L = w[pos + 5], w[pos + 6]
            at = pos + 12
            self.entries.append(dict(chip=w[pos], column=w[pos + 1], kind="relation" if w[pos + 2] else "constant", l0=w[pos + 3], support=w[pos + 4],
                                     terms=[(w[at + 2 * i], w[at + 2 * i + 1]) for i in range(T)], enforced_rows=u64(pos + 8), free_rows=u64(pos + 10),
                                     rows=w[at + 2 * T:at + 2 * T + L]))
            pos = at + 2 * T + L
        assert pos == len(w)

    def _columns(self, chip, keep):
        return [e["column"] for e in self.entries if e["chip"] == chip and keep(e)]

    def constant_columns(self, chip):
        """The listed columns of `chip` that hold one value on every row."""
        return self._columns(chip, lambda e: e["kind"] == "constant")

    def relations(self, chip):
        """The listed columns of `chip` that are an affine function of earlier columns (and not constant)."""
        return self._columns(chip, lambda e: e["kind"] == "relation")

    def never_enforced(self, chip):
        """The listed columns of `chip` whose invariant no row's constraints and records enforce: candidates for a missing constraint."""
        return self._columns(chip, lambda e: e["enforced_rows"] == 0)

    def holds(self, main_matrices):
        """The (chip, column) pairs of the listed entries whose relation FAILS on some row of the given canonical traces (one matrix per chip;
        plain numpy, no library call): [] on the audited witness, and a way to test one witness's invariants against another program's traces.
        Raises for an entry whose vector was cut at max_terms."""
        bad = []
        for e in self.entries:
            if e["support"] > len(e["terms"]):
                raise VgpuError(-1, "invariant_audit: the vector of chip %d column %d is cut (%d terms, %d listed): it cannot be evaluated" %
                                (e["chip"], e["column"], e["support"], len(e["terms"])))
            m = np.asarray(main_matrices[e["chip"]], dtype=np.uint64)
            acc = np.full(m.shape[0], e["l0"], dtype=np.uint64)
            for col, coef in e["terms"]:
                acc = (acc + m[:, col] % np.uint64(P) * np.uint64(coef)) % np.uint64(P)
            if acc.any():
                bad.append((e["chip"], e["column"]))
        return bad

    def to_dict(self):
        return dict(max_terms=self.max_terms, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms,
                    host_ms=self.host_ms, evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _invariant_opts(max_entries, max_rows_per_entry, max_terms, chips):
    # as _rank_opts: explicit zeros are refused here, with the library's status code
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1 or int(max_terms) < 1:
        raise VgpuError(-1, "invariant_audit: max_entries, max_rows_per_entry and max_terms must be at least 1")
    return InvariantAuditOpts(int(max_entries), int(max_rows_per_entry), _chip_mask("invariant", chips), int(max_terms), (ctypes.c_uint32 * 3)(0, 0, 0))


def invariant_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None):
    """The invariant audit on the HOST (vgpu_invariant_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], max_terms = the (column, coefficient) terms listed per invariant, chips = the chip indices to audit
    (default: all); an InvariantReport back."""
    opts = _invariant_opts(max_entries, max_rows_per_entry, max_terms, chips)
    return _audit_host("invariant", machine, main_matrices, preprocessed, opts)


class ProductAuditOpts(ctypes.Structure):  # vgpu_product_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("max_terms", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 3)]


PRODUCT_KINDS = ("boolean", "zero", "select", "other")


class ProductReport(_AuditReport):
    """The product audit of a witness (vgpu_product_audit / vgpu_product_audit_host; the contract is stated in include/vgpu.h), as plain Python
    values: max_terms, truncated, total_entries (the relations of the audited chips), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, rank (rho), independent (q = rho - 1), pairs (m), relations, boolean,
    zero, select, other (counts), every, some, never (relations enforced on every row, on some rows, on no row))],
    entries = [dict(chip, i, j, kind ("boolean" / "zero" / "select" / "other"), b0, support, terms=[(column, coefficient)], enforced_rows,
    free_rows, flat_rows, rows=[the first free rows])] ascending by (chip, i, j): M[r][i] * M[r][j] = b0 + sum(coefficient * M[r][column]) on
    every row r of the witness,
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations of the enforcement phase).
    Single products, one row, THIS witness, first order: candidates for missing constraints, not findings."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31525156 or w[1] != len(w):
            raise ValueError("not a product report image")
        self.words = np.array(w, dtype=np.uint32)
        self.max_terms = w[2]
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 8
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), rank=w[pos + 6],
                                   independent=max(w[pos + 6], 1) - 1, pairs=w[pos + 7], relations=w[pos + 8], boolean=w[pos + 9], zero=w[pos + 10], select=w[pos + 11],
                                   other=w[pos + 12], every=w[pos + 13], some=w[pos + 14], never=w[pos + 15]))
            pos += 16
        self.entries = []
        for _ in range(self.reported):
            T, L = w[pos + 6], w[pos + 7]
            at = pos + 16
            self.entries.append(dict(chip=w[pos], i=w[pos + 1], j=w[pos + 2], kind=PRODUCT_KINDS[w[pos + 3]], b0=w[pos + 4], support=w[pos + 5],
                                     terms=[(w[at + 2 * k], w[at + 2 * k + 1]) for k in range(T)], enforced_rows=u64(pos + 8), free_rows=u64(pos + 10),
                                     flat_rows=u64(pos + 12), rows=w[at + 2 * T:at + 2 * T + L]))
            pos = at + 2 * T + L
        assert pos == len(w)

    def _pairs(self, chip, keep):
        return [(e["i"], e["j"]) for e in self.entries if e["chip"] == chip and keep(e)]

    def relations(self, chip):
        """The listed pairs (i, j) of `chip` whose product is an affine function of the row."""
        return self._pairs(chip, lambda e: True)

    def never_enforced(self, chip):
        """The listed pairs of `chip` whose relation no row's constraints and records enforce: candidates for a missing constraint."""
        return self._pairs(chip, lambda e: e["enforced_rows"] == 0)

    def holds(self, main_matrices):
        """The (chip, i, j) of the listed entries whose relation FAILS on some row of the given canonical traces (one matrix per chip; plain
        numpy, no library call): [] on the audited witness, and a way to test one witness's relations against another program's traces.
        Raises for an entry whose beta was cut at max_terms."""
        bad = []
        for e in self.entries:
            if e["support"] > len(e["terms"]):
                raise VgpuError(-1, "product_audit: the beta of chip %d pair (%d, %d) is cut (%d terms, %d listed): it cannot be evaluated" %
                                (e["chip"], e["i"], e["j"], e["support"], len(e["terms"])))
            m = np.asarray(main_matrices[e["chip"]], dtype=np.uint64) % np.uint64(P)
            acc = np.full(m.shape[0], e["b0"], dtype=np.uint64)
            for col, coef in e["terms"]:
                acc = (acc + m[:, col] * np.uint64(coef)) % np.uint64(P)
            if (acc != m[:, e["i"]] * m[:, e["j"]] % np.uint64(P)).any():
                bad.append((e["chip"], e["i"], e["j"]))
        return bad

    def to_dict(self):
        return dict(max_terms=self.max_terms, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms,
                    host_ms=self.host_ms, evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _product_opts(max_entries, max_rows_per_entry, max_terms, chips):
    # as _rank_opts: explicit zeros are refused here, with the library's status code
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1 or int(max_terms) < 1:
        raise VgpuError(-1, "product_audit: max_entries, max_rows_per_entry and max_terms must be at least 1")
    return ProductAuditOpts(int(max_entries), int(max_rows_per_entry), _chip_mask("product", chips), int(max_terms), (ctypes.c_uint32 * 3)(0, 0, 0))


def product_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None):
    """The product audit on the HOST (vgpu_product_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], max_terms = the (column, coefficient) terms listed per relation, chips = the chip indices to audit
    (default: all); a ProductReport back."""
    opts = _product_opts(max_entries, max_rows_per_entry, max_terms, chips)
    return _audit_host("product", machine, main_matrices, preprocessed, opts)


class DomainAuditOpts(ctypes.Structure):  # vgpu_domain_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("max_bits", ctypes.c_uint32),
                ("lookup_auto", ctypes.c_uint32), ("lookup_global_mask", ctypes.c_uint64), ("lookup_local_mask", ctypes.c_uint64), ("reserved", ctypes.c_uint32 * 2)]


DOMAIN_CLASSES = ("constant", "boolean", "byte", "half", "wide")


class DomainReport(_AuditReport):
    """The domain audit of a witness (vgpu_domain_audit / vgpu_domain_audit_host; the contract is stated in include/vgpu.h), as plain Python
    values: max_bits, lookup_auto, truncated, total_entries (the narrow columns with an unguarded non-zero row), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, is_table, narrow, entries, appearances)],
    columns(chip) = [dict(column, min, max, distinct_narrow, cls ("constant" / "boolean" / "byte" / "half" / "wide"), dense, bits, narrow,
    appearances, nonzero_rows, wide_rows, guarded_rows, sent_rows, received_rows, unguarded_rows, unguarded_nonzero_rows, mixed_rows)] ([] for a
    chip that is not audited),
    buses = [dict(bus, is_global, bus_index, lookup, width, positions=[dict(position, is_send, lookup, min, max, distinct_narrow, wide_records,
    records)])] ascending by (is_global, bus_index), per position the sends, then the receives,
    entries = [dict(chip, column, cls, max, unguarded_nonzero_rows, appearances=[dict(interaction, position, is_send, is_global, bus_index, lookup,
    live_rows)], rows=[(row, value)])] ascending by (chip, column),
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (cells scanned).
    THIS witness only, bare fields only: candidates for a missing range check, not findings."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 12 or w[0] != 0x314d4456 or w[1] != len(w):
            raise ValueError("not a domain report image")
        self.words = np.array(w, dtype=np.uint32)
        self.max_bits, self.truncated = w[2], bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.lookup_auto = bool(w[8])
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 12
        self.chips, self._columns = [], []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), is_table=bool(w[pos + 6]),
                                   narrow=w[pos + 7], entries=w[pos + 8], appearances=w[pos + 9]))
            audited, width = bool(w[pos + 3]), w[pos]
            pos += 10
            cols = []
            for k in range(width):
                if audited:
                    cols.append(dict(column=k, min=w[pos], max=w[pos + 1], distinct_narrow=w[pos + 2], cls=DOMAIN_CLASSES[w[pos + 3]], dense=bool(w[pos + 4]), bits=w[pos + 5],
                                     narrow=bool(w[pos + 6]), appearances=w[pos + 7], nonzero_rows=u64(pos + 8), wide_rows=u64(pos + 10), guarded_rows=u64(pos + 12),
                                     sent_rows=u64(pos + 14), received_rows=u64(pos + 16), unguarded_rows=u64(pos + 18), unguarded_nonzero_rows=u64(pos + 20), mixed_rows=u64(pos + 22)))
                pos += 24
            self._columns.append(cols)
        self.buses = []
        for b in range(w[9]):
            self.buses.append(dict(bus=b, is_global=bool(w[pos]), bus_index=w[pos + 1], lookup=bool(w[pos + 2]), width=w[pos + 3], positions=[]))
            pos += 4
        for _ in range(w[10]):
            self.buses[w[pos]]["positions"].append(dict(position=w[pos + 1], is_send=bool(w[pos + 2]), lookup=bool(w[pos + 3]), min=w[pos + 4], max=w[pos + 5], distinct_narrow=w[pos + 6],
                                                        wide_records=u64(pos + 8), records=u64(pos + 10)))
            pos += 12
        self.entries = []
        for _ in range(self.reported):
            A, L = w[pos + 4], w[pos + 5]
            at = pos + 8
            apps = [dict(interaction=w[at + 8 * k], position=w[at + 8 * k + 1], is_send=bool(w[at + 8 * k + 2]), is_global=bool(w[at + 8 * k + 3]), bus_index=w[at + 8 * k + 4],
                         lookup=bool(w[at + 8 * k + 5]), live_rows=u64(at + 8 * k + 6)) for k in range(A)]
            at += 8 * A
            self.entries.append(dict(chip=w[pos], column=w[pos + 1], cls=DOMAIN_CLASSES[w[pos + 2]], max=w[pos + 3], unguarded_nonzero_rows=u64(pos + 6), appearances=apps,
                                     rows=[(w[at + 2 * k], w[at + 2 * k + 1]) for k in range(L)]))
            pos = at + 2 * L
        assert pos == len(w)

    def columns(self, chip):
        """The column records of `chip` ([] when it was not audited)."""
        return self._columns[chip]

    def unguarded(self, chip):
        """The listed columns of `chip` that are narrow and hold a non-zero cell on a row with no live bare send to a lookup bus."""
        return [e["column"] for e in self.entries if e["chip"] == chip]

    def lookup_buses(self):
        """[(is_global, bus_index)] of the buses counted as lookup tables."""
        return [(b["is_global"], b["bus_index"]) for b in self.buses if b["lookup"]]

    def to_dict(self):
        return dict(max_bits=self.max_bits, lookup_auto=self.lookup_auto, truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms,
                    host_ms=self.host_ms, evaluations=self.evaluations, chips=self.chips, columns=self._columns, buses=self.buses, entries=self.entries)


def _domain_opts(max_entries, max_rows_per_entry, chips, max_bits, lookup_buses):
    """lookup_buses: None (the structural rule) or a list of (is_global, bus_index) pairs / bare global bus indices that count as lookup tables."""
    if int(max_entries) < 0 or int(max_rows_per_entry) < 0 or int(max_bits) < 1:
        raise VgpuError(-1, "domain_audit: max_entries and max_rows_per_entry must not be negative, max_bits at least 1")
    gmask = lmask = 0
    if lookup_buses is not None:
        for b in lookup_buses:
            is_global, index = (True, int(b)) if isinstance(b, (int, np.integer)) else (bool(b[0]), int(b[1]))
            if index < 0 or index > 63:
                raise VgpuError(-1, "domain_audit: lookup_buses names bus indices below 64")
            if is_global:
                gmask |= 1 << index
            else:
                lmask |= 1 << index
    return DomainAuditOpts(int(max_entries), int(max_rows_per_entry), _chip_mask("domain", chips), int(max_bits), 1 if lookup_buses is None else 0, gmask, lmask, (ctypes.c_uint32 * 2)(0, 0))


def domain_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None, max_bits=16, lookup_buses=None):
    """The domain audit on the HOST (vgpu_domain_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], chips = the chip indices to audit (default: all), max_bits = a column is narrow below 2^max_bits,
    lookup_buses = None (the structural rule) or the buses that count as lookup tables; a DomainReport back."""
    opts = _domain_opts(max_entries, max_rows_per_entry, chips, max_bits, lookup_buses)
    return _audit_host("domain", machine, main_matrices, preprocessed, opts)


class MemoryAuditOpts(ctypes.Structure):  # vgpu_memory_audit_opts_t
    _fields_ = [("max_findings", ctypes.c_uint32), ("bus_is_global", ctypes.c_uint32), ("bus_index", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


MEMORY_KINDS = ("malformed", "duplicate_static", "stale_read", "uninit_read")
MEMORY_COUNTERS = ("slots", "live", "reads", "writes", "statics", "addresses", "min_addr", "max_addr", "max_clk", "max_clk_gap", "uninit_zero_reads", "same_cycle_pairs", "dummy_reads_clk",
                   "dummy_reads_addr", "layout_descents", "findings") + MEMORY_KINDS


class MemoryReport(_AuditReport):
    """The memory audit of a witness (vgpu_memory_audit / vgpu_memory_audit_host; the contract is stated in include/vgpu.h), as plain Python
    values: words (the image), bus = (is_global, bus_index), max_findings, truncated, receives = [(chip, interaction)],
    counters = dict(slots, live, reads, writes, statics, addresses, min_addr, max_addr, max_clk, max_clk_gap, uninit_zero_reads, same_cycle_pairs,
    dummy_reads_clk, dummy_reads_addr, layout_descents, findings, malformed, duplicate_static, stale_read, uninit_read),
    first_descent = (chip, row) of the first layout descent or None,
    findings = [dict(kind ("malformed" / "duplicate_static" / "stale_read" / "uninit_read"), reason, chip, interaction, row, addr, clk, value,
    expected, last_write = (chip, interaction, row) or None, position)] in ascending order position,
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (slots evaluated).
    It judges the table's receives of THIS witness; whether the senders agree is the bus audit's question."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 48 or w[0] != 0x314d4d56 or w[1] != len(w):
            raise ValueError("not a memory report image")
        self.words = np.array(w, dtype=np.uint32)
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        self.bus = (bool(w[2]), w[3])
        self.truncated, self.max_findings = bool(w[5]), w[7]
        self.counters = dict(slots=u64(8), live=u64(10), reads=u64(12), writes=u64(14), statics=u64(16), addresses=u64(18), min_addr=w[20], max_addr=w[21], max_clk=w[22], max_clk_gap=w[23],
                             uninit_zero_reads=u64(24), same_cycle_pairs=u64(26), dummy_reads_clk=u64(28), dummy_reads_addr=u64(30), layout_descents=u64(32), findings=u64(36),
                             malformed=u64(38), duplicate_static=u64(40), stale_read=u64(42), uninit_read=u64(44))
        self.first_descent = None if w[34] == 0xFFFFFFFF else (w[34], w[35])
        pos = 48
        self.receives = [(w[pos + 2 * k], w[pos + 2 * k + 1]) for k in range(w[4])]
        pos += 2 * w[4]
        self.findings = []
        for _ in range(w[6]):
            f = w[pos:pos + 20]
            self.findings.append(dict(kind=MEMORY_KINDS[f[0] - 1], reason=f[1], chip=f[2], interaction=f[3], row=f[4], addr=f[5], clk=f[6], value=f[7:11], expected=f[11:15],
                                      last_write=None if f[15] == 0xFFFFFFFF else (f[15], f[16], f[17]), position=f[18]))
            pos += 20
        assert pos == len(w)

    @property
    def total_findings(self):
        return self.counters["findings"]

    def to_dict(self):
        return dict(words=[int(x) for x in self.words], bus=list(self.bus), max_findings=self.max_findings, truncated=self.truncated, receives=[list(r) for r in self.receives],
                    counters=self.counters, first_descent=None if self.first_descent is None else list(self.first_descent),
                    findings=[dict(f, last_write=None if f["last_write"] is None else list(f["last_write"])) for f in self.findings], device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations)

    @classmethod
    def from_dict(cls, d):
        """The report of to_dict()'s object (a `check --memory` JSON report's "memory" key)."""
        return cls(d["words"], d.get("device_ms", 0.0), d.get("host_ms", 0.0), d.get("evaluations", 0.0))


def _memory_opts(max_findings, bus):
    """bus: None (global bus 2, the BasicMachine's memory bus), a global bus index, or (is_global, bus_index)."""
    if int(max_findings) < 0 or int(max_findings) >= 1 << 32:
        raise VgpuError(-1, "memory_audit: max_findings must not be negative")
    is_global, index = (True, 2) if bus is None else ((True, int(bus)) if isinstance(bus, (int, np.integer)) else (bool(bus[0]), int(bus[1])))
    if index < 0 or index >= 1 << 32:
        raise VgpuError(-1, "memory_audit: bus names a bus index")
    return MemoryAuditOpts(int(max_findings), 1 if is_global else 0, index, 0)


def memory_audit_host(machine, main_matrices, preprocessed, max_findings=64, bus=None):
    """The memory audit on the HOST (vgpu_memory_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], bus = None (global bus 2), a global bus index or (is_global, bus_index); a MemoryReport back."""
    return _audit_host("memory", machine, main_matrices, preprocessed, _memory_opts(max_findings, bus))


class ProgramAuditOpts(ctypes.Structure):  # vgpu_program_audit_opts_t
    _fields_ = [("fetch_chip", ctypes.c_uint32), ("pc_col", ctypes.c_uint32), ("n_fields", ctypes.c_uint32), ("field_cols", ctypes.c_uint32 * 8), ("table_chip", ctypes.c_uint32),
                ("key_col", ctypes.c_uint32), ("table_cols", ctypes.c_uint32 * 8), ("mult_col", ctypes.c_uint32), ("rom_len", ctypes.c_uint32), ("max_findings", ctypes.c_uint32),
                ("max_ranges", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


PROGRAM_KINDS = ("table_key", "pc_out_of_rom", "wrong_instruction", "wrapped_operand", "multiplicity")
PROGRAM_HARD_KINDS = ("table_key", "pc_out_of_rom", "wrong_instruction", "multiplicity")
PROGRAM_COUNTERS = ("fetches", "table_rows", "rom_len", "fetched_words", "unfetched_words", "unfetched_ranges", "hottest_pc", "hottest_count", "first_pc", "last_pc", "sequential", "stay",
                    "jumps", "hard") + PROGRAM_KINDS
PROGRAM_TWO32 = (1 << 32) % P  # what the unsigned and the signed embedding of one negative i32 differ by


class ProgramReport(_AuditReport):
    """The program audit of a witness (vgpu_program_audit / vgpu_program_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: words (the image), fetch_chip, table_chip, n_fields, max_findings, max_ranges, truncated = (findings, wrapped, unfetched),
    counters = dict(fetches, table_rows, rom_len, fetched_words, unfetched_words, unfetched_ranges, hottest_pc, hottest_count, first_pc,
    last_pc, sequential, stay, jumps, hard, table_key, pc_out_of_rom, wrong_instruction, wrapped_operand, multiplicity),
    hard = the listed hard findings and wrapped = the listed wrapped-operand rows, each [dict(kind, mask, fields = the field indices of mask,
    row, pc, found, expected)] (for table_key and multiplicity row = pc = the table row, found[0] = the key or the multiplicity,
    expected[0] = the row or the fetch count mod p, expected[1] = the fetch count), unfetched = [(lo, hi)],
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (fetches + table rows).
    It judges the fetches against the table of THIS witness; wrapped operands are never a fault."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 48 or w[0] != 0x31475056 or w[1] != len(w) or len(w) != 48 + 24 * (w[6] + w[7]) + 2 * w[8]:
            raise ValueError("not a program report image")
        self.words = np.array(w, dtype=np.uint32)
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        self.fetch_chip, self.table_chip, self.n_fields, self.max_findings, self.max_ranges = w[2], w[3], w[4], w[9], w[10]
        self.truncated = (bool(w[5] & 1), bool(w[5] & 2), bool(w[5] & 4))
        self.counters = dict(fetches=u64(12), table_rows=u64(14), rom_len=w[11], fetched_words=u64(16), unfetched_words=u64(18), unfetched_ranges=u64(20), hottest_pc=w[22],
                             hottest_count=u64(24), first_pc=w[26], last_pc=w[27], sequential=u64(28), stay=u64(30), jumps=u64(32), hard=u64(34), table_key=u64(36), pc_out_of_rom=u64(38),
                             wrong_instruction=u64(40), wrapped_operand=u64(42), multiplicity=u64(44))
        pos = 48
        self.hard, self.wrapped = [], []
        for n, into in ((w[6], self.hard), (w[7], self.wrapped)):
            for _ in range(n):
                f = w[pos:pos + 24]
                into.append(dict(kind=PROGRAM_KINDS[f[0] - 1], mask=f[1], fields=[j for j in range(8) if f[1] >> j & 1], row=f[2], pc=f[3], found=f[4:12], expected=f[12:20]))
                pos += 24
        self.unfetched = [(w[pos + 2 * k], w[pos + 2 * k + 1]) for k in range(w[8])]

    @property
    def total_hard(self):
        return self.counters["hard"]

    @property
    def total_wrapped(self):
        return self.counters["wrapped_operand"]

    def to_dict(self):
        return dict(words=[int(x) for x in self.words], fetch_chip=self.fetch_chip, table_chip=self.table_chip, n_fields=self.n_fields, max_findings=self.max_findings,
                    max_ranges=self.max_ranges, truncated=list(self.truncated), counters=self.counters, hard=self.hard, wrapped=self.wrapped, unfetched=[list(r) for r in self.unfetched],
                    device_ms=self.device_ms, host_ms=self.host_ms, evaluations=self.evaluations)

    @classmethod
    def from_dict(cls, d):
        """The report of to_dict()'s object (a `check --program` JSON report's "program" key)."""
        return cls(d["words"], d.get("device_ms", 0.0), d.get("host_ms", 0.0), d.get("evaluations", 0.0))


def _program_opts(rom_len, max_findings, max_ranges, fetch, table):
    """fetch: None (the BasicMachine's cpu: chip 0, pc column 1, field columns 3..8) or (chip, pc_col, [field columns]); table: None (its
    program chip: chip 1, key column 0, word columns 1..6, multiplicity column 0) or (chip, key_col, [word columns], mult_col)."""
    fchip, pc_col, fcols = (0, 1, [3, 4, 5, 6, 7, 8]) if fetch is None else (int(fetch[0]), int(fetch[1]), [int(c) for c in fetch[2]])
    tchip, key_col, tcols, mult_col = (1, 0, [1, 2, 3, 4, 5, 6], 0) if table is None else (int(table[0]), int(table[1]), [int(c) for c in table[2]], int(table[3]))
    if len(fcols) != len(tcols):
        raise VgpuError(-1, "program_audit: the fetching chip and the table name as many field columns (%d, %d)" % (len(fcols), len(tcols)))
    if not 1 <= len(fcols) <= 8:
        raise VgpuError(-1, "program_audit: n_fields is 1 to 8 (got %d)" % len(fcols))
    values = [fchip, pc_col, tchip, key_col, mult_col, int(rom_len), int(max_findings), int(max_ranges)] + fcols + tcols
    if any(v < 0 or v >= 1 << 32 for v in values):
        raise VgpuError(-1, "program_audit: chips, columns, rom_len and the limits are not negative")
    u8 = ctypes.c_uint32 * 8
    return ProgramAuditOpts(fchip, pc_col, len(fcols), u8(*fcols), tchip, key_col, u8(*tcols), mult_col, int(rom_len), int(max_findings), int(max_ranges), 0)


def program_audit_host(machine, main_matrices, preprocessed, rom_len=0, max_findings=64, max_ranges=64, fetch=None, table=None):
    """The program audit on the HOST (vgpu_program_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], rom_len = the ROM's length (0: the table's height; Workload.program_len is a VM witness's),
    fetch = None or (chip, pc_col, [field columns]), table = None or (chip, key_col, [word columns], mult_col); a ProgramReport back."""
    return _audit_host("program", machine, main_matrices, preprocessed, _program_opts(rom_len, max_findings, max_ranges, fetch, table))


class ArithmeticAuditOpts(ctypes.Structure):  # vgpu_arithmetic_audit_opts_t
    _fields_ = [("max_findings", ctypes.c_uint32), ("bus_is_global", ctypes.c_uint32), ("bus_index", ctypes.c_uint32), ("sides", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


ARITHMETIC_OPCODES = ("ADD32", "SUB32", "MUL32", "DIV32", "LT32", "SHL32", "SHR32", "AND32", "OR32", "XOR32", "SDIV32", "NE32", "MULHU32", "SRA32", "MULHS32", "LTE32", "EQ32", "SLT32",
                      "SLE32")  # opcode 100 + index
ARITHMETIC_KINDS = ("malformed", "undefined", "wrong_result", "shift_quotient", "arithmetic_shr")
ARITHMETIC_HARD_KINDS = ARITHMETIC_KINDS[:3]
ARITHMETIC_SOFT_KINDS = ARITHMETIC_KINDS[3:]
ARITHMETIC_REASONS = ("division_by_zero", "signed_overflow", "shift_range")
ARITHMETIC_COUNTERS = ("slots", "live", "judged", "other", "hard", "malformed", "undefined", "wrong_result", "soft", "shift_quotient", "arithmetic_shr", "mulhs_sign_matters") + ARITHMETIC_REASONS
ARITHMETIC_SIDES = dict(receives=1, sends=2, both=3)


class ArithmeticReport(_AuditReport):
    """The arithmetic audit of a witness (vgpu_arithmetic_audit / vgpu_arithmetic_audit_host; the contract is stated in include/vgpu.h), as
    plain Python values: words (the image), bus = (is_global, bus_index), sides, max_findings, truncated = (hard, soft),
    counters = dict(slots, live, judged, other, hard, malformed, undefined, wrong_result, soft, shift_quotient, arithmetic_shr,
    mulhs_sign_matters, division_by_zero, signed_overflow, shift_range), opcodes = dict(name -> judged records),
    entries = [dict(chip, interaction, is_send, n_fields, live, hard)], hard = the listed hard findings and soft = the listed soft ones, each
    [dict(kind, mask (the reason of an undefined record), chip, interaction, row, opcode, x, y, z (four bytes each, most significant first),
    expected (the word the opcode computes; 0 for malformed and undefined), count, is_send)], device_ms (the device pass; 0.0 for the host
    audit), host_ms (the whole call), evaluations (the live records).  It judges each record alone; soft findings are never a fault."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 80 or w[0] != 0x31524156 or w[1] != len(w) or len(w) != 80 + 8 * w[9] + 24 * (w[6] + w[7]):
            raise ValueError("not an arithmetic report image")
        self.words = np.array(w, dtype=np.uint32)
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        self.bus, self.sides, self.max_findings = (bool(w[2]), w[3]), w[4], w[8]
        self.truncated = (bool(w[5] & 1), bool(w[5] & 2))
        self.counters = {name: u64(10 + 2 * k) for k, name in enumerate(ARITHMETIC_COUNTERS)}
        self.opcodes = {name: u64(40 + 2 * k) for k, name in enumerate(ARITHMETIC_OPCODES)}
        pos = 80
        self.entries = []
        for _ in range(w[9]):
            self.entries.append(dict(chip=w[pos], interaction=w[pos + 1], is_send=bool(w[pos + 2]), n_fields=w[pos + 3], live=u64(pos + 4), hard=u64(pos + 6)))
            pos += 8
        self.hard, self.soft = [], []
        for n, into in ((w[6], self.hard), (w[7], self.soft)):
            for _ in range(n):
                f = w[pos:pos + 24]
                into.append(dict(kind=ARITHMETIC_KINDS[f[0] - 1], mask=f[1], chip=f[2], interaction=f[3], row=f[4], opcode=f[5], x=f[6:10], y=f[10:14], z=f[14:18], expected=f[18],
                                 count=f[19], is_send=bool(f[20])))
                pos += 24

    @property
    def total_hard(self):
        return self.counters["hard"]

    @property
    def total_soft(self):
        return self.counters["soft"]

    def to_dict(self):
        return dict(words=[int(x) for x in self.words], bus=list(self.bus), sides=self.sides, max_findings=self.max_findings, truncated=list(self.truncated), counters=self.counters,
                    opcodes=self.opcodes, entries=self.entries, hard=self.hard, soft=self.soft, device_ms=self.device_ms, host_ms=self.host_ms, evaluations=self.evaluations)

    @classmethod
    def from_dict(cls, d):
        """The report of to_dict()'s object (a `check --arithmetic` JSON report's "arithmetic" key)."""
        return cls(d["words"], d.get("device_ms", 0.0), d.get("host_ms", 0.0), d.get("evaluations", 0.0))


def _arithmetic_opts(max_findings, bus, sides):
    """bus: None (global bus 0, the BasicMachine's general bus), a global bus index, or (is_global, bus_index); sides: "receives", "sends",
    "both" or the bit set itself (bit 0 receives, bit 1 sends)."""
    if int(max_findings) < 0 or int(max_findings) >= 1 << 32:
        raise VgpuError(-1, "arithmetic_audit: max_findings must not be negative")
    is_global, index = (True, 0) if bus is None else ((True, int(bus)) if isinstance(bus, (int, np.integer)) else (bool(bus[0]), int(bus[1])))
    if index < 0 or index >= 1 << 32:
        raise VgpuError(-1, "arithmetic_audit: bus names a bus index")
    if isinstance(sides, str):
        if sides not in ARITHMETIC_SIDES:
            raise VgpuError(-1, "arithmetic_audit: sides is receives, sends or both (got %r)" % sides)
        sides = ARITHMETIC_SIDES[sides]
    if int(sides) < 0 or int(sides) >= 1 << 32:
        raise VgpuError(-1, "arithmetic_audit: sides is 1 (receives), 2 (sends) or 3 (both)")
    return ArithmeticAuditOpts(int(max_findings), 1 if is_global else 0, index, int(sides), 0)


def arithmetic_audit_host(machine, main_matrices, preprocessed, max_findings=64, bus=None, sides="receives"):
    """The arithmetic audit on the HOST (vgpu_arithmetic_audit_host: no device, one thread): main_matrices = one canonical matrix per chip,
    preprocessed = [(chip index, matrix)], bus = None (global bus 0), a global bus index or (is_global, bus_index), sides = "receives", "sends"
    or "both"; an ArithmeticReport back."""
    return _audit_host("arithmetic", machine, main_matrices, preprocessed, _arithmetic_opts(max_findings, bus, sides))


class TransitionAuditOpts(ctypes.Structure):  # vgpu_transition_audit_opts_t
    _fields_ = [("max_entries", ctypes.c_uint64), ("max_rows_per_entry", ctypes.c_uint32), ("chip_mask", ctypes.c_uint32), ("max_terms", ctypes.c_uint32),
                ("min_gate_windows", ctypes.c_uint32), ("max_gates", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class TransitionReport(_AuditReport):
    """The transition audit of a witness (vgpu_transition_audit / vgpu_transition_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: max_terms, min_gate_windows, max_gates, truncated, total_entries, reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, n_bool, n_gates, gates_listed, gates_audited, rank (rho_0), dim (d_0),
    local_only, next_only, transitions (d_0 split three ways), gated (entries of the gates >= 1))],
    gates = [dict(chip, column, value, audited, windows, rank, dim, entries)] (column 0: gate 0, every window),
    entries = [dict(chip, gate=(window column, value) or None, column f, kind ("constant" / "one_block" / "both_blocks"), l0, support,
    terms=[(window column, coefficient)], free_windows, held_windows, rows=[the first free windows])] ascending by (chip, gate, column):
    l0 + sum(coefficient * a_r[window column]) = 0 on every window r of the gate, a_r = (1, M[r], M[r + 1]): window column 1 + c is `local`
    column c, 1 + width + c is `next` column c.
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations of the verdicts).
    Affine-linear, single gates, THIS witness, per basis vector, first order and one row at a time: candidates for missing transition
    constraints, not findings."""

    KINDS = ("constant", "one_block", "both_blocks")

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 12 or w[0] != 0x31525456 or w[1] != len(w):
            raise ValueError("not a transition report image")
        self.words = np.array(w, dtype=np.uint32)
        self.max_terms = w[2]
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.min_gate_windows, self.max_gates = w[9], w[10]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 12
        self.chips = []
        for c in range(w[7]):
            self.chips.append(dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), n_bool=w[pos + 6],
                                   n_gates=w[pos + 7], gates_listed=w[pos + 8], gates_audited=w[pos + 9], rank=w[pos + 10], dim=w[pos + 11], local_only=w[pos + 12],
                                   next_only=w[pos + 13], transitions=w[pos + 14], gated=w[pos + 15]))
            pos += 16
        self.gates = []
        for _ in range(w[8]):
            self.gates.append(dict(chip=w[pos], column=w[pos + 1], value=w[pos + 2], audited=bool(w[pos + 3]), windows=u64(pos + 4), rank=w[pos + 6], dim=w[pos + 7],
                                   entries=w[pos + 8]))
            pos += 10
        self.entries = []
        for _ in range(self.reported):
            T, L = w[pos + 7], w[pos + 8]
            at = pos + 14
            self.entries.append(dict(chip=w[pos], gate=(w[pos + 1], w[pos + 2]) if w[pos + 1] else None, column=w[pos + 3], kind=self.KINDS[w[pos + 4]], l0=w[pos + 5],
                                     support=w[pos + 6], terms=[(w[at + 2 * i], w[at + 2 * i + 1]) for i in range(T)], free_windows=u64(pos + 10),
                                     held_windows=u64(pos + 12), rows=w[at + 2 * T:at + 2 * T + L]))
            pos = at + 2 * T + L
        assert pos == len(w)

    def name_of(self, chip, window_column):
        """'1', 'local[c]' or 'next[c]' for a window column of `chip`."""
        W = self.chips[chip]["width"]
        if window_column == 0:
            return "1"
        return "local[%d]" % (window_column - 1) if window_column <= W else "next[%d]" % (window_column - 1 - W)

    def never_held(self, chip):
        """The listed entries of `chip` that no window of their gate holds: candidates for a missing transition constraint."""
        return [e for e in self.entries if e["chip"] == chip and e["held_windows"] == 0]

    def holds(self, main_matrices):
        """The (chip, gate, column) triples of the listed entries whose relation FAILS on some window of its gate in the given canonical traces (one
        matrix per chip; plain numpy, no library call): [] on the audited witness, and a way to test one witness's relations against another
        program's traces.  Raises for an entry whose vector was cut at max_terms."""
        bad = []
        for e in self.entries:
            if e["support"] > len(e["terms"]):
                raise VgpuError(-1, "transition_audit: the vector of chip %d gate %s column %d is cut (%d terms, %d listed): it cannot be evaluated" %
                                (e["chip"], e["gate"], e["column"], e["support"], len(e["terms"])))
            m = np.asarray(main_matrices[e["chip"]], dtype=np.uint64) % np.uint64(P)
            if m.shape[0] < 2:
                continue
            a = np.concatenate([np.ones((m.shape[0] - 1, 1), dtype=np.uint64), m[:-1], m[1:]], axis=1)  # the windows
            acc = np.full(a.shape[0], e["l0"], dtype=np.uint64)
            for col, coef in e["terms"]:
                acc = (acc + a[:, col] * np.uint64(coef)) % np.uint64(P)
            if e["gate"] is not None:
                acc = acc[a[:, e["gate"][0]] == np.uint64(e["gate"][1])]
            if acc.any():
                bad.append((e["chip"], e["gate"], e["column"]))
        return bad

    def to_dict(self):
        return dict(max_terms=self.max_terms, min_gate_windows=self.min_gate_windows, max_gates=self.max_gates, truncated=self.truncated, total_entries=self.total_entries,
                    reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms, evaluations=self.evaluations, chips=self.chips, gates=self.gates, entries=self.entries)


def _transition_opts(max_entries, max_rows_per_entry, max_terms, min_gate_windows, max_gates, chips):
    # as _rank_opts: explicit zeros are refused here, with the library's status code
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1 or int(max_terms) < 1 or int(min_gate_windows) < 1 or int(max_gates) < 1:
        raise VgpuError(-1, "transition_audit: max_entries, max_rows_per_entry, max_terms, min_gate_windows and max_gates must be at least 1")
    if int(min_gate_windows) > 0xFFFFFFFF or int(max_gates) > 0xFFFFFFFF or int(max_terms) > 0xFFFFFFFF:
        raise VgpuError(-1, "transition_audit: max_terms, min_gate_windows and max_gates are 32-bit counts")
    return TransitionAuditOpts(int(max_entries), int(max_rows_per_entry), _chip_mask("transition", chips), int(max_terms), int(min_gate_windows), int(max_gates),
                               (ctypes.c_uint32 * 3)(0, 0, 0))


def transition_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, min_gate_windows=64, max_gates=256, chips=None):
    """The transition audit on the HOST (vgpu_transition_audit_host: no device, one thread, no width limit): main_matrices = one canonical
    matrix per chip, preprocessed = [(chip index, matrix)], max_terms = the (window column, coefficient) terms listed per entry,
    min_gate_windows = the fewest windows of an audited gate, max_gates = the gates listed per chip, chips = the chip indices to audit (default:
    all); a TransitionReport back."""
    opts = _transition_opts(max_entries, max_rows_per_entry, max_terms, min_gate_windows, max_gates, chips)
    return _audit_host("transition", machine, main_matrices, preprocessed, opts)


class FieldReport(_AuditReport):
    """The field audit of a witness (vgpu_field_audit / vgpu_field_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    truncated, total_entries ((chip, interaction, field) with a floating row), reported,
    chips = [dict(chip, width, constraints, interactions, audited, height, live_records, floating_fields, floating_rows (sums over the rows),
    records=[dict(interaction, is_send, is_global, bus_index, fields, live_rows, constant=[flag per field], floating=[rows per field])])],
    entries = [dict(chip, interaction, field, floating, rows=[dict(row, n_support, terms=[(column, coefficient)])])] ascending,
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations).
    First order, THIS witness, the other rows' cells held fixed; a floating field on a send usually means that the chip delegates."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31414656 or w[1] != len(w) or w[2] != 8:
            raise ValueError("not a field report image")
        self.words = np.array(w, dtype=np.uint32)
        self.truncated = bool(w[3])
        self.total_entries, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 8
        self.chips = []
        for c in range(w[7]):
            chip = dict(chip=c, width=w[pos], constraints=w[pos + 1], interactions=w[pos + 2], audited=bool(w[pos + 3]), height=u64(pos + 4), live_records=u64(pos + 6),
                        floating_fields=u64(pos + 8), floating_rows=u64(pos + 10), records=[])
            pos += 12
            for m in range(chip["interactions"]):
                nf = w[pos + 3]
                chip["records"].append(dict(interaction=m, is_send=bool(w[pos]), is_global=bool(w[pos + 1]), bus_index=w[pos + 2], fields=nf, live_rows=u64(pos + 4),
                                            constant=[bool(w[pos + 6 + 3 * j]) for j in range(nf)], floating=[u64(pos + 7 + 3 * j) for j in range(nf)]))
                pos += 6 + 3 * nf
            self.chips.append(chip)
        self.entries = []
        for _ in range(self.reported):
            rows = []
            for k in range(w[pos + 3]):
                at = pos + 6 + 18 * k
                rows.append(dict(row=w[at], n_support=w[at + 1], terms=[(w[at + 2 + 2 * i], w[at + 3 + 2 * i]) for i in range(min(8, w[at + 1]))]))
            self.entries.append(dict(chip=w[pos], interaction=w[pos + 1], field=w[pos + 2], floating=u64(pos + 4), rows=rows))
            pos += 6 + 18 * w[pos + 3]
        assert pos == len(w)

    def floating(self, chip):
        """{(interaction, field): rows where the field floats} of `chip`, the fields that float on some row (exact, from the per-field counts)."""
        return {(r["interaction"], j): n for r in self.chips[chip]["records"] for j, n in enumerate(r["floating"]) if n}

    def to_dict(self):
        return dict(truncated=self.truncated, total_entries=self.total_entries, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, entries=self.entries)


def _field_opts(max_entries, max_rows_per_entry, chips):
    # the rank audit's options (vgpu_rank_audit_opts_t) and refusals, under this audit's name
    if int(max_entries) < 1 or int(max_rows_per_entry) < 1:
        raise VgpuError(-1, "field_audit: max_entries and max_rows_per_entry must be at least 1")
    if chips is not None and (not list(chips) or any(int(c) < 0 or int(c) > 31 for c in chips)):
        raise VgpuError(-1, "field_audit: chips is a non-empty list of chip indices below 32")
    return _rank_opts(max_entries, max_rows_per_entry, chips)


def field_audit_host(machine, main_matrices, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
    """The field audit on the HOST (vgpu_field_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)], chips = the chip indices to audit (default: all); a FieldReport back."""
    opts = _field_opts(max_entries, max_rows_per_entry, chips)
    return _audit_host("field", machine, main_matrices, preprocessed, opts)


class LinkAuditOpts(ctypes.Structure):  # vgpu_link_audit_opts_t
    _fields_ = [("max_tuples", ctypes.c_uint64), ("max_records_per_tuple", ctypes.c_uint32), ("hash_bits", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class LinkReport(_AuditReport):
    """The link audit of a witness (vgpu_link_audit / vgpu_link_audit_host; the contract is stated in include/vgpu.h), as plain Python values:
    truncated, open_tuples (tuples with an open position: exact even when the list is cut), reported,
    buses = [dict(bus=(is_global, bus_index), width, live, tuples, open_tuples, open_in=[tuples in which position j is open], open_records=[the
    records of those])],
    chips = [dict(chip, records=[dict(interaction, is_send, is_global, bus_index, fields, live_rows, constant=[flag per field], floating=[rows
    per field], open=[rows per field])])],
    tuples = [dict(bus, mask, open=[the open positions], n_send, n_recv, fields, records=[(chip, row, interaction, is_send, record mask)])] in
    the order of their first records,
    device_ms (the device pass; 0.0 for the host audit), host_ms (the whole call), evaluations (dual row evaluations of the masks).
    First order, THIS witness, every record judged alone: open means that no single record's own chip pins the position."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 8 or w[0] != 0x31414C56 or w[1] != len(w):
            raise ValueError("not a link report image")
        self.words = np.array(w, dtype=np.uint32)
        self.truncated = bool(w[2])
        self.open_tuples, self.reported = w[3] | (w[4] << 32), w[5]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 8
        self.buses = []
        for _ in range(w[6]):
            width = w[pos + 2]
            self.buses.append(dict(bus=(w[pos], w[pos + 1]), width=width, live=u64(pos + 3), tuples=u64(pos + 5), open_tuples=u64(pos + 7),
                                   open_in=[u64(pos + 9 + 4 * j) for j in range(width)], open_records=[u64(pos + 11 + 4 * j) for j in range(width)]))
            pos += 9 + 4 * width
        self.chips = []
        for c in range(w[7]):
            chip = dict(chip=c, records=[])
            n_inter = w[pos]
            pos += 1
            for m in range(n_inter):
                nf = w[pos + 3]
                chip["records"].append(dict(interaction=m, is_send=bool(w[pos]), is_global=bool(w[pos + 1]), bus_index=w[pos + 2], fields=nf, live_rows=u64(pos + 4),
                                            constant=[bool(w[pos + 6 + 5 * j]) for j in range(nf)], floating=[u64(pos + 7 + 5 * j) for j in range(nf)],
                                            open=[u64(pos + 9 + 5 * j) for j in range(nf)]))
                pos += 6 + 5 * nf
            self.chips.append(chip)
        self.tuples = []
        for _ in range(self.reported):
            width, mask, n_listed = w[pos + 2], w[pos + 3], w[pos + 8]
            t = dict(bus=(w[pos], w[pos + 1]), mask=mask, open=[j for j in range(width) if (mask >> j) & 1], n_send=u64(pos + 4), n_recv=u64(pos + 6), fields=w[pos + 9:pos + 9 + width])
            pos += 9 + width
            t["records"] = [tuple(w[pos + 5 * k:pos + 5 * k + 5]) for k in range(n_listed)]
            pos += 5 * n_listed
            self.tuples.append(t)
        assert pos == len(w)

    def open(self, chip):
        """{(interaction, field): (floating rows, open rows)} of `chip`, the fields that float on some row: a floating row that is not open is
        answered (another record of its tuple pins the field)."""
        return {(r["interaction"], j): (n, r["open"][j]) for r in self.chips[chip]["records"] for j, n in enumerate(r["floating"]) if n}

    def to_dict(self):
        return dict(truncated=self.truncated, open_tuples=self.open_tuples, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms, evaluations=self.evaluations,
                    buses=[dict(b, bus=list(b["bus"])) for b in self.buses], chips=self.chips,
                    tuples=[dict(t, bus=list(t["bus"]), records=[list(r) for r in t["records"]]) for t in self.tuples])


def _link_opts(max_tuples, max_records_per_tuple, hash_bits):
    # in the C struct a zero field selects its default, so the refusals of explicit zeros are made here, with the library's status code
    if not 1 <= int(hash_bits) <= 64:
        raise VgpuError(-1, "link_audit: hash_bits must be 1..64")
    if int(max_tuples) < 1 or int(max_records_per_tuple) < 1:
        raise VgpuError(-1, "link_audit: max_tuples and max_records_per_tuple must be at least 1")
    return LinkAuditOpts(int(max_tuples), int(max_records_per_tuple), int(hash_bits), 0)


def link_audit_host(machine, main_matrices, preprocessed, max_tuples=64, max_records_per_tuple=4, hash_bits=64):
    """The link audit on the HOST (vgpu_link_audit_host: no device, one thread): main_matrices = one canonical matrix per chip, preprocessed =
    [(chip index, matrix)]; a LinkReport back.  hash_bits is accepted for symmetry with Prover.link_audit (the host groups by full tuples)."""
    opts = _link_opts(max_tuples, max_records_per_tuple, hash_bits)
    return _audit_host("link", machine, main_matrices, preprocessed, opts)


class CoverageAuditOpts(ctypes.Structure):  # vgpu_coverage_audit_opts_t
    _fields_ = [("max_cells", ctypes.c_uint64), ("n_deltas", ctypes.c_uint32), ("deltas", ctypes.c_uint32 * 4), ("max_workgroups", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 2)]


NO_ROW = 0xFFFFFFFF


class CoverageReport(_AuditReport):
    """The coverage audit of a witness (vgpu_coverage_audit / vgpu_coverage_audit_host; the contract is stated in include/vgpu.h), as plain
    Python values: deltas, truncated, total_cells ((chip, detector, column, delta) with kills > 0), reported,
    chips = [dict(chip, width, constraints, interactions, height, dead_constraints, shadowed_constraints, dead_interactions,
    shadowed_interactions (numbers), detected=[per delta], free=[..], kills=[[per delta] per detector], sole=[..])] (sums over the chip's columns),
    cells = [dict(chip, detector, column, delta, kills, sole, first_row, first_sole_row)] ascending by (chip, detector, column, delta index),
    device_ms, host_ms, evaluations.  Detectors 0..K-1 are the constraints, K..K+M-1 the interactions.  "Dead" and "shadowed" speak of this
    witness and of single-cell mutations by these deltas only: neither is a fault, and shadowed does not mean removable."""

    def __init__(self, words, device_ms=0.0, host_ms=0.0, evaluations=0.0):
        w = [int(x) for x in words]
        if len(w) < 12 or w[0] != 0x31524B56 or w[1] != len(w) or not 1 <= w[2] <= 4:
            raise ValueError("not a coverage report image")
        self.words = np.array(w, dtype=np.uint32)
        D = w[2]
        self.deltas, self.truncated = w[8:8 + D], bool(w[3])
        self.total_cells, self.reported = w[4] | (w[5] << 32), w[6]
        self.device_ms, self.host_ms, self.evaluations = float(device_ms), float(host_ms), float(evaluations)

        def u64(at):
            return w[at] | (w[at + 1] << 32)

        pos = 12
        self.chips = []
        for c in range(w[7]):
            K, M = w[pos + 1], w[pos + 2]
            at = pos + 10 + 4 * D
            self.chips.append(dict(chip=c, width=w[pos], constraints=K, interactions=M, height=u64(pos + 4), dead_constraints=w[pos + 6], shadowed_constraints=w[pos + 7],
                                   dead_interactions=w[pos + 8], shadowed_interactions=w[pos + 9], detected=[u64(pos + 10 + 4 * i) for i in range(D)],
                                   free=[u64(pos + 12 + 4 * i) for i in range(D)], kills=[[u64(at + 4 * (t * D + i)) for i in range(D)] for t in range(K + M)],
                                   sole=[[u64(at + 4 * (t * D + i) + 2) for i in range(D)] for t in range(K + M)]))
            pos = at + 4 * D * (K + M)
        self.cells = []
        for _ in range(self.reported):
            self.cells.append(dict(chip=w[pos], detector=w[pos + 1], column=w[pos + 2], delta=w[pos + 3], kills=u64(pos + 4), sole=u64(pos + 6), first_row=w[pos + 8],
                                   first_sole_row=w[pos + 9]))
            pos += 10
        assert pos == len(w)

    def _split(self, chip, pred):
        c = self.chips[chip]
        K = c["constraints"]
        hit = [t for t in range(K + c["interactions"]) if pred(sum(c["kills"][t]), sum(c["sole"][t]))]
        return [t for t in hit if t < K], [t - K for t in hit if t >= K]

    def dead(self, chip):
        """(constraints, interactions) of `chip` that no mutation of any cell makes fail / changes: indices, the interactions counted from 0."""
        return self._split(chip, lambda k, s: k == 0)

    def shadowed(self, chip):
        """(constraints, interactions) of `chip` that detect some mutation and are never the only detector of one."""
        return self._split(chip, lambda k, s: k > 0 and s == 0)

    def essential(self, chip):
        return self._split(chip, lambda k, s: s > 0)

    def to_dict(self):
        return dict(deltas=self.deltas, truncated=self.truncated, total_cells=self.total_cells, reported=self.reported, device_ms=self.device_ms, host_ms=self.host_ms,
                    evaluations=self.evaluations, chips=self.chips, cells=self.cells)

    @staticmethod
    def _image(deltas, truncated, total_cells, chips, cells):
        def u64(v):
            return [v & 0xFFFFFFFF, v >> 32]

        D = len(deltas)
        w = [0x31524B56, 0, D, int(truncated)] + u64(total_cells) + [len(cells), len(chips)] + (list(deltas) + [0] * 4)[:4]
        for c in chips:
            w += [c["width"], c["constraints"], c["interactions"], 0] + u64(c["height"])
            w += [c["dead_constraints"], c["shadowed_constraints"], c["dead_interactions"], c["shadowed_interactions"]]
            for i in range(D):
                w += u64(c["detected"][i]) + u64(c["free"][i])
            for t in range(c["constraints"] + c["interactions"]):
                for i in range(D):
                    w += u64(c["kills"][t][i]) + u64(c["sole"][t][i])
        for e in cells:
            w += [e["chip"], e["detector"], e["column"], e["delta"]] + u64(e["kills"]) + u64(e["sole"]) + [e["first_row"], e["first_sole_row"]]
        w[1] = len(w)
        return np.array(w, dtype=np.uint32)

    @classmethod
    def from_dict(cls, d):
        """The report of to_dict()'s object (a `check --coverage` JSON report's "coverage" key)."""
        return cls(cls._image(d["deltas"], d["truncated"], d["total_cells"], d["chips"], d["cells"]), d.get("device_ms", 0.0), d.get("host_ms", 0.0), d.get("evaluations", 0.0))

    @classmethod
    def merge(cls, reports):
        """The corpus-level report of several witnesses of ONE machine audited with ONE delta set: kills, sole, detected and free add cell-wise,
        heights add, the classes are recomputed, and the row minima are dropped (0xFFFFFFFF: rows of different witnesses do not compare).
        Reports of differing machines or deltas, and cut ones (their cell lists are not whole), are refused."""
        reports = list(reports)
        if not reports:
            raise ValueError("merge: no report")
        first = reports[0]
        shape = [(c["width"], c["constraints"], c["interactions"]) for c in first.chips]
        D = len(first.deltas)
        chips = [dict(c, height=0, detected=[0] * D, free=[0] * D, kills=[[0] * D for _ in c["kills"]], sole=[[0] * D for _ in c["sole"]]) for c in first.chips]
        cells = {}
        for r in reports:
            if r.deltas != first.deltas:
                raise ValueError("merge: the reports were made with different deltas")
            if [(c["width"], c["constraints"], c["interactions"]) for c in r.chips] != shape:
                raise ValueError("merge: the reports are of different machines")
            if r.truncated:
                raise ValueError("merge: a report's cell list was cut (max_cells)")
            for c, m in zip(r.chips, chips):
                m["height"] += c["height"]
                for i in range(D):
                    m["detected"][i] += c["detected"][i]
                    m["free"][i] += c["free"][i]
                for t in range(len(m["kills"])):
                    for i in range(D):
                        m["kills"][t][i] += c["kills"][t][i]
                        m["sole"][t][i] += c["sole"][t][i]
            for e in r.cells:
                key = (e["chip"], e["detector"], e["column"], e["delta"])
                k, s = cells.get(key, (0, 0))
                cells[key] = (k + e["kills"], s + e["sole"])
        for m in chips:
            K = m["constraints"]
            cls_of = ["dead" if sum(k) == 0 else "shadowed" if sum(s) == 0 else "essential" for k, s in zip(m["kills"], m["sole"])]
            m["dead_constraints"], m["shadowed_constraints"] = cls_of[:K].count("dead"), cls_of[:K].count("shadowed")
            m["dead_interactions"], m["shadowed_interactions"] = cls_of[K:].count("dead"), cls_of[K:].count("shadowed")
        listed = [dict(chip=key[0], detector=key[1], column=key[2], delta=key[3], kills=k, sole=s, first_row=NO_ROW, first_sole_row=NO_ROW) for key, (k, s) in sorted(cells.items())]
        return cls(cls._image(first.deltas, False, len(listed), chips, listed))


def _coverage_opts(deltas, max_cells, max_workgroups):
    # as _mutation_opts: explicit zeros and an empty delta list are refused here, with the library's status code
    if int(max_cells) < 1:
        raise VgpuError(-1, "coverage_audit: max_cells must be at least 1")
    ds = [int(d) for d in ((1, P - 1) if deltas is None else deltas)]
    if not 1 <= len(ds) <= 4:
        raise VgpuError(-1, "coverage_audit: 1 to 4 deltas (got %d)" % len(ds))
    if any(d < 0 or d > 0xFFFFFFFF for d in ds):
        raise VgpuError(-1, "coverage_audit: a delta must be a canonical value in 1..p-1")
    if not 0 <= int(max_workgroups) <= 0xFFFFFFFF:
        raise VgpuError(-1, "coverage_audit: max_workgroups is a 32-bit count (0: the default)")
    return CoverageAuditOpts(int(max_cells), len(ds), (ctypes.c_uint32 * 4)(*ds), int(max_workgroups), (ctypes.c_uint32 * 2)(0, 0))


def coverage_audit_host(machine, main_matrices, preprocessed, deltas=None, max_cells=8192):
    """The coverage audit on the HOST (vgpu_coverage_audit_host: no device, one thread, no limits): main_matrices = one canonical matrix per
    chip, preprocessed = [(chip index, matrix)], deltas = 1 to 4 distinct values in 1..p-1 (default (1, p - 1)); a CoverageReport back."""
    opts = _coverage_opts(deltas, max_cells, 0)
    return _audit_host("coverage", machine, main_matrices, preprocessed, opts)


_AUDIT_REPORTS = dict(bus=BusReport, constraint=ConstraintReport, mutation=MutationReport, pair=PairReport, rank=RankReport, step=StepReport, invariant=InvariantReport, transition=TransitionReport, product=ProductReport, domain=DomainReport, memory=MemoryReport, program=ProgramReport, arithmetic=ArithmeticReport, field=FieldReport,
                      link=LinkReport, coverage=CoverageReport)


def _report_of(name):
    return lambda h: _audit_report(name, _AUDIT_REPORTS[name], h)


# a raw vgpu_X_audit(_host) call's handle as the audit's report (the tests of the options structs call the C entry points themselves)
_rank_report, _step_report, _field_report, _link_report = _report_of("rank"), _report_of("step"), _report_of("field"), _report_of("link")

def _pool_poison_from_env(environ):
    """The pool-poison word of VGPU_POOL_POISON (decimal or 0x hex, 0 .. 2^32 - 1), or None when the variable is unset or empty (off)."""
    text = environ.get("VGPU_POOL_POISON", "").strip()
    if not text:
        return None
    hexa = text[:2] in ("0x", "0X")
    digits = text[2:] if hexa else text
    if not digits or any(ch not in ("0123456789abcdefABCDEF" if hexa else "0123456789") for ch in digits):  # no sign, no underscores, no spaces
        raise ValueError("VGPU_POOL_POISON must be a 32-bit word in decimal or 0x hex, not %r" % text)
    word = int(digits, 16 if hexa else 10)
    if word > 0xFFFFFFFF:
        raise ValueError("VGPU_POOL_POISON must be a 32-bit word (at most 0xFFFFFFFF), not %r" % text)
    return word


class Ticket:
    """An outstanding asynchronous proof (vgpu_prove_async); keeps its inputs alive until waited for."""

    def __init__(self, handle, keep):
        self._h, self._keep = handle, keep

    def wait(self):
        h = ctypes.c_void_p()
        t, self._h = self._h, None
        _check(lib().vgpu_ticket_wait(t, ctypes.byref(h)))
        self._keep = None
        return Proof(h)

    def __del__(self):
        if getattr(self, "_h", None):  # never leave a worker thread using freed traces behind
            try:
                self.wait()
            except Exception:
                pass


class Prover:
    """One MI355X: StarkConfig + Machine -> prove().  Mirrors machine.prove(&config)."""

    def __init__(self, machine, rc, device=0, log_blowup=1, num_queries=40, pow_bits=8, observe_final_poly=False, interpret_air=False, hash_kind=HASH_KECCAK256):
        cfg = VgpuConfig()
        cfg.device, cfg.log_blowup, cfg.num_queries, cfg.pow_bits = device, log_blowup, num_queries, pow_bits
        cfg.hash_kind, cfg.observe_final_poly, cfg.interpret_air = int(hash_kind), int(observe_final_poly), int(interpret_air)
        rc = np.ascontiguousarray(rc, dtype=np.uint32)
        assert rc.size == 480
        ctypes.memmove(cfg.poseidon_rc, rc.ctypes.data, 480 * 4)
        self.machine, self.rc, self.log_blowup, self.num_queries, self.pow_bits = machine, rc, log_blowup, num_queries, pow_bits
        self._h = ctypes.c_void_p()
        # the dense lane's switch, read once, here: VGPU_DENSE_LANE=0 turns it off for this context (A/B runs, parity tests),
        # VGPU_DENSE_LANE_MIN_NODES sets the smallest tree that takes it (the tests' small trees); parsed before the context exists
        lane_off, lane_min = os.environ.get("VGPU_DENSE_LANE", "1") == "0", os.environ.get("VGPU_DENSE_LANE_MIN_NODES", "").strip()
        if lane_min and not lane_min.isdigit():
            raise ValueError("VGPU_DENSE_LANE_MIN_NODES must be a number of leaf rows, not %r" % lane_min)
        poison = _pool_poison_from_env(os.environ)  # a test switch (set_pool_poison), read once, here
        _check(lib().vgpu_prover_create(ctypes.byref(cfg), machine._h, ctypes.byref(self._h)))
        if lane_off or int(lane_min or 0) > 0:
            self.set_dense_lane(not lane_off, int(lane_min or 0))
        if os.environ.get("VGPU_CONST_COLS", "1") == "0":  # the constant-column switch (on in the library), read once, here: A/B runs, parity tests
            self.set_const_columns(False)
        if poison is not None:
            self.set_pool_poison(poison)

    def set_const_columns(self, on):
        """vgpu_prover_set_const_columns: fill the constant columns of uploaded main / preprocessed traces in the LDE instead of transforming them."""
        lib().vgpu_prover_set_const_columns(self._h, ctypes.c_uint32(1 if on else 0))

    def set_dense_lane(self, on, min_nodes=0):
        """vgpu_prover_set_dense_lane: the device's dense lane on / off for this context; min_nodes > 0 = the smallest tree that takes it."""
        lib().vgpu_prover_set_dense_lane(self._h, ctypes.c_uint32(1 if on else 0), ctypes.c_uint64(int(min_nodes)))

    def upload(self, matrix):
        m = np.ascontiguousarray(matrix, dtype=np.uint32)
        assert m.ndim == 2
        h = ctypes.c_void_p()
        _check(lib().vgpu_trace_upload(self._h, m.ctypes.data_as(c_u32p), ctypes.c_uint64(m.shape[0]), ctypes.c_uint64(m.shape[1]), ctypes.byref(h)))
        return DeviceTrace(self, h, m.shape)

    def upload_oplog(self, desc):
        h = ctypes.c_void_p()
        _check(lib().vgpu_oplog_upload(self._h, ctypes.byref(desc), ctypes.byref(h)))
        nbytes = 48 * desc.n_cpu + 16 * desc.n_mem + 16 * sum(desc.n_alu) + 8 * desc.n_static
        log = DeviceOplog(self, h, int(nbytes))
        log._desc = desc
        return log

    def generate_trace(self, log, chip):
        """Chip::generate_trace of `chip` on the device, from the uploaded operation logs."""
        h = ctypes.c_void_p()
        _check(lib().vgpu_generate_trace(self._h, log._h, ctypes.c_uint32(chip), ctypes.byref(h)))
        hh, ww = ctypes.c_uint64(), ctypes.c_uint64()
        lib().vgpu_trace_shape(h, ctypes.byref(hh), ctypes.byref(ww))
        return DeviceTrace(self, h, (int(hh.value), int(ww.value)))

    def commit_batches(self, traces, coset_shifts=None):
        arr = (ctypes.c_void_p * len(traces))(*[t._h for t in traces])
        root = np.zeros(8, dtype=np.uint32)
        sh = None
        if coset_shifts is not None:
            shv, sh = _u32(coset_shifts)
        h = ctypes.c_void_p()
        _check(lib().vgpu_commit_batches(self._h, arr, ctypes.c_uint32(len(traces)), sh, root.ctypes.data_as(c_u32p), ctypes.byref(h)))
        return ProverData(self, h, root, [t.shape for t in traces])

    def commit_batches_flagged(self, traces):
        """vgpu_commit_batches_flagged (a test hook): the main round's commitment as prove() runs it — constant columns found by the ingest and, with
        the switch on, filled by the LDE.  Returns (ProverData, flags): flags[i][j] != 0 iff column j of matrix i is not constant."""
        arr = (ctypes.c_void_p * len(traces))(*[t._h for t in traces])
        root = np.zeros(8, dtype=np.uint32)
        varies = np.zeros(sum(t.shape[1] for t in traces), dtype=np.uint32)
        h = ctypes.c_void_p()
        _check(lib().vgpu_commit_batches_flagged(self._h, arr, ctypes.c_uint32(len(traces)), root.ctypes.data_as(c_u32p), ctypes.byref(h), varies.ctypes.data_as(c_u32p)))
        return ProverData(self, h, root, [t.shape for t in traces]), np.split(varies, np.cumsum([t.shape[1] for t in traces])[:-1])

    def generate_permutation_trace(self, chip, main, challenges, preprocessed=None):
        info = self.machine.chip_info(chip)
        n = main.shape[0]
        out = np.zeros((n, 5 * (info["interactions"] + 1)), dtype=np.uint32)
        ch, chp = _u32(challenges)
        cs = np.zeros(5, dtype=np.uint32)
        _check(lib().vgpu_perm_trace(self._h, ctypes.c_uint32(chip), main._h, preprocessed._h if preprocessed is not None else None, chp,
                                     out.ctypes.data_as(c_u32p), ctypes.c_uint64(out.size), cs.ctypes.data_as(c_u32p)))
        return out, cs

    def permutation_trace_device(self, chip, main, challenges, preprocessed=None):
        """generate_permutation_trace left in HBM: (DeviceTrace, cumulative_sum[5])."""
        ch, chp = _u32(challenges)
        cs = np.zeros(5, dtype=np.uint32)
        h = ctypes.c_void_p()
        _check(lib().vgpu_perm_trace_device(self._h, ctypes.c_uint32(chip), main._h, preprocessed._h if preprocessed is not None else None, chp, ctypes.byref(h),
                                            cs.ctypes.data_as(c_u32p)))
        hh, ww = ctypes.c_uint64(), ctypes.c_uint64()
        lib().vgpu_trace_shape(h, ctypes.byref(hh), ctypes.byref(ww))
        return DeviceTrace(self, h, (int(hh.value), int(ww.value))), cs

    def quotient(self, chip, main_pd, main_idx, perm_pd, perm_idx, perm_challenges, alpha, cumulative_sum, prep_pd=None, prep_idx=0):
        """quotient + decompose_and_flatten of one chip from its committed LDEs -> DeviceTrace of the chunk matrix (n x 10)."""
        a, ap = _u32(perm_challenges)
        b, bp = _u32(alpha)
        c, cp = _u32(cumulative_sum)
        h = ctypes.c_void_p()
        _check(lib().vgpu_quotient(self._h, ctypes.c_uint32(chip), prep_pd._h if prep_pd is not None else None, ctypes.c_uint32(prep_idx), main_pd._h,
                                   ctypes.c_uint32(main_idx), perm_pd._h, ctypes.c_uint32(perm_idx), ap, bp, cp, ctypes.byref(h)))
        hh, ww = ctypes.c_uint64(), ctypes.c_uint64()
        lib().vgpu_trace_shape(h, ctypes.byref(hh), ctypes.byref(ww))
        return DeviceTrace(self, h, (int(hh.value), int(ww.value)))

    def open_multi_batches(self, rounds, points, challenger):
        """pcs.open_multi_batches: rounds = [ProverData]; points[r][i] = list of Ext5 (5 words) for matrix i of round r.
        Returns (openings[r][i][p] as (width, 5) arrays, TwoAdicFriPcsProof words); advances `challenger`."""
        arr = (ctypes.c_void_p * len(rounds))(*[r._h for r in rounds])
        n_points = np.array([len(pts) for rnd in points for pts in rnd], dtype=np.uint32)
        flat = np.array([w for rnd in points for pts in rnd for z in pts for w in z], dtype=np.uint32)
        h = ctypes.c_void_p()
        _check(lib().vgpu_open_multi_batches(self._h, arr, ctypes.c_uint32(len(rounds)), n_points.ctypes.data_as(c_u32p), flat.ctypes.data_as(c_u32p), challenger._h,
                                             ctypes.byref(h)))
        L = lib()
        for f in (L.vgpu_opening_values_len, L.vgpu_opening_proof_len):
            f.restype = ctypes.c_uint64
        for f in (L.vgpu_opening_values, L.vgpu_opening_proof):
            f.restype = c_u32p
        try:
            nv, npf = int(L.vgpu_opening_values_len(h)), int(L.vgpu_opening_proof_len(h))
            vals = np.ctypeslib.as_array(L.vgpu_opening_values(h), shape=(nv,)).copy() if nv else np.zeros(0, np.uint32)
            proof = np.ctypeslib.as_array(L.vgpu_opening_proof(h), shape=(npf,)).copy()
        finally:
            L.vgpu_opening_free(h)
        out, pos = [], 0
        for r, rnd in enumerate(points):
            out.append([])
            for i, pts in enumerate(rnd):
                w = rounds[r]._shapes[i][1]
                out[r].append([])
                for _ in pts:
                    out[r][i].append(vals[pos:pos + 5 * w].reshape(w, 5))
                    pos += 5 * w
        assert pos == vals.size
        return out, proof

    def fri_fold(self, f, beta):
        f = np.ascontiguousarray(f, dtype=np.uint32)
        n = f.shape[0]
        b, bp = _u32(beta)
        out = np.zeros((n // 2, 5), dtype=np.uint32)
        _check(lib().vgpu_fri_fold(self._h, f.ctypes.data_as(c_u32p), ctypes.c_uint64(n), bp, out.ctypes.data_as(c_u32p)))
        return out

    def prove(self, main, preprocessed, debug=False, check=False):
        """main: list of DeviceTrace (chip order); preprocessed: list of (chip index, DeviceTrace).
        check: evaluate every constraint on the traces first (the reference's debug-build check_constraints)."""
        arr = (ctypes.c_void_p * len(main))(*[t._h for t in main])
        chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
        parr = (ctypes.c_void_p * max(1, len(preprocessed)))(*[t._h for _, t in preprocessed])
        h = ctypes.c_void_p()
        _check(lib().vgpu_prove(self._h, arr, ctypes.c_uint32(len(main)), chips, parr, ctypes.c_uint32(len(preprocessed)),
                                ctypes.c_uint32((1 if debug else 0) | (2 if check else 0)), ctypes.byref(h)))
        return Proof(h)

    def _audit(self, name, main, preprocessed, opts):
        """vgpu_`name`_audit: the arguments of prove and the audit's options; the audit's report back."""
        arr = (ctypes.c_void_p * max(1, len(main)))(*[t._h for t in main])
        chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
        parr = (ctypes.c_void_p * max(1, len(preprocessed)))(*[t._h for _, t in preprocessed])
        h = ctypes.c_void_p()
        _check(getattr(lib(), "vgpu_%s_audit" % name)(self._h, arr, ctypes.c_uint32(len(main)), chips, parr, ctypes.c_uint32(len(preprocessed)), ctypes.byref(opts), ctypes.byref(h)))
        return _audit_report(name, _AUDIT_REPORTS[name], h)

    def bus_audit(self, main, preprocessed, max_tuples=64, max_records_per_tuple=4, hash_bits=64):
        """Which bus tuples of this witness are unbalanced (vgpu_bus_audit; the exact form of check_cumulative_sums): the arguments of prove,
        a BusReport back.  hash_bits < 64 is a test hook (the grouping key is cut; the report must not change)."""
        opts = _bus_opts(max_tuples, max_records_per_tuple, hash_bits)
        return self._audit("bus", main, preprocessed, opts)

    def constraint_audit(self, main, preprocessed, max_constraints=64, max_rows_per_constraint=4):
        """Which AIR constraints of this witness fail, on which rows, with which value (vgpu_constraint_audit; check_constraints made exact and
        complete): the arguments of prove, a ConstraintReport back."""
        opts = _constraint_opts(max_constraints, max_rows_per_constraint)
        return self._audit("constraint", main, preprocessed, opts)

    def mutation_audit(self, main, preprocessed, deltas=None, max_entries=1024, max_rows_per_entry=4):
        """Which cells of this witness could be changed by a delta without any AIR constraint or bus noticing (vgpu_mutation_audit; mutation
        testing of the AIRs): the arguments of prove, deltas = 1 to 4 distinct values in 1..p-1 (default (1, p - 1)); a MutationReport back."""
        opts = _mutation_opts(deltas, max_entries, max_rows_per_entry)
        return self._audit("mutation", main, preprocessed, opts)

    def pair_audit(self, main, preprocessed, deltas=None, max_entries=1024, max_rows_per_entry=4, chips=None):
        """Which two cells of one row of this witness could be changed together without any AIR constraint or bus noticing although one of the
        changes alone is noticed (vgpu_pair_audit): the arguments of prove, deltas as in mutation_audit, chips = the chip indices to audit
        (default: all); a PairReport back."""
        opts = _pair_opts(deltas, max_entries, max_rows_per_entry, chips)
        return self._audit("pair", main, preprocessed, opts)

    def rank_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
        """Every first-order degree of freedom of each trace row of this witness (vgpu_rank_audit): per row the null space of the Jacobian of
        all constraints and bus records that read the row; the arguments of prove, chips = the chip indices to audit (default: all); a
        RankReport back."""
        opts = _rank_opts(max_entries, max_rows_per_entry, chips)
        return self._audit("rank", main, preprocessed, opts)

    def step_audit(self, main, preprocessed, steps=None, max_entries=1024, max_rows_per_entry=4, chips=None):
        """Finite steps along each row's null directions (vgpu_step_audit): the rank audit's canonical null vector of every (row, loose column),
        moved by each step and judged by the mutation audit's rule; the arguments of prove, steps = 1 to 4 distinct canonical values (default 1,
        p - 1, 2), chips = the chip indices to audit (default: all); a StepReport back."""
        opts = _step_opts(steps, max_entries, max_rows_per_entry, chips)
        return self._audit("step", main, preprocessed, opts)

    def invariant_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None):
        """The affine-linear relations every row of each chip of this witness keeps, and on how many rows the chip's own constraints and bus
        records enforce each of them to first order (vgpu_invariant_audit); the arguments of prove, max_terms = the (column, coefficient) terms
        listed per invariant, chips = the chip indices to audit (default: all); an InvariantReport back."""
        opts = _invariant_opts(max_entries, max_rows_per_entry, max_terms, chips)
        return self._audit("invariant", main, preprocessed, opts)

    def product_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, chips=None):
        """Which products of two independent columns this witness keeps an affine function of the row, and on which rows the chip's constraints
        and records enforce each relation to first order (vgpu_product_audit); the arguments of prove, max_terms = the (column, coefficient)
        terms listed per relation, chips = the chip indices to audit (default: all); a ProductReport back."""
        opts = _product_opts(max_entries, max_rows_per_entry, max_terms, chips)
        return self._audit("product", main, preprocessed, opts)

    def domain_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None, max_bits=16, lookup_buses=None):
        """Which set of values this witness puts into every main column, and on which rows a narrow (byte or half-word valued) column is not a
        field of a live send to a lookup table (vgpu_domain_audit); the arguments of prove, chips = the chip indices to audit (default: all),
        max_bits = a column is narrow below 2^max_bits, lookup_buses = None (the structural rule) or the buses that count as lookup tables; a
        DomainReport back."""
        opts = _domain_opts(max_entries, max_rows_per_entry, chips, max_bits, lookup_buses)
        return self._audit("domain", main, preprocessed, opts)

    def memory_audit(self, main, preprocessed, max_findings=64, bus=None):
        """Whether the receives of the memory bus of this witness are a memory: every read returns the last value written to its address
        (vgpu_memory_audit); the arguments of prove, bus = None (global bus 2), a global bus index or (is_global, bus_index); a MemoryReport
        back with the records that break it and the exact counters."""
        return self._audit("memory", main, preprocessed, _memory_opts(max_findings, bus))

    def program_audit(self, main, preprocessed, rom_len=0, max_findings=64, max_ranges=64, fetch=None, table=None):
        """Whether the instruction fetches of this witness match its program ROM and the ROM's multiplicities match the fetch counts
        (vgpu_program_audit); the arguments of prove, rom_len = the ROM's length (0: the table's height; Workload.program_len is a VM
        witness's), fetch = None (the cpu) or (chip, pc_col, [field columns]), table = None (the program chip) or (chip, key_col, [word
        columns], mult_col); a ProgramReport back with the fetches and table rows that break the would-be program bus and the exact counters."""
        return self._audit("program", main, preprocessed, _program_opts(rom_len, max_findings, max_ranges, fetch, table))

    def arithmetic_audit(self, main, preprocessed, max_findings=64, bus=None, sides="receives"):
        """Whether the ALU records of this witness compute their opcode (vgpu_arithmetic_audit); the arguments of prove, bus = None (global
        bus 0, the general bus), a global bus index or (is_global, bus_index), sides = "receives", "sends" or "both"; an ArithmeticReport back
        with the records whose stored result is not what their opcode computes and the exact counters."""
        return self._audit("arithmetic", main, preprocessed, _arithmetic_opts(max_findings, bus, sides))

    def transition_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, max_terms=8, min_gate_windows=64, max_gates=256, chips=None):
        """Which affine-linear relations between a row and its successor this witness keeps, on every window or under a boolean gate, and at
        which windows the chip's constraints and records hold each of them to first order (vgpu_transition_audit); the arguments of prove,
        max_terms = the (window column, coefficient) terms listed per entry, min_gate_windows = the fewest windows of an audited gate, max_gates
        = the gates listed per chip, chips = the chip indices to audit (default: all); a TransitionReport back."""
        opts = _transition_opts(max_entries, max_rows_per_entry, max_terms, min_gate_windows, max_gates, chips)
        return self._audit("transition", main, preprocessed, opts)

    def field_audit(self, main, preprocessed, max_entries=1024, max_rows_per_entry=4, chips=None):
        """Which fields of the chips' bus records this witness's constraints leave undetermined (vgpu_field_audit): per row and live record,
        is each field fixed to first order by the constraints, the counts and the record's other fields; the arguments of prove, chips = the
        chip indices to audit (default: all); a FieldReport back."""
        opts = _field_opts(max_entries, max_rows_per_entry, chips)
        return self._audit("field", main, preprocessed, opts)

    def link_audit(self, main, preprocessed, max_tuples=64, max_records_per_tuple=4, hash_bits=64):
        """Which positions of this witness's bus tuples no chip on the bus pins (vgpu_link_audit): the field audit's float mask of every live
        record, ANDed over the records of each tuple of the bus audit; the arguments of prove, a LinkReport back.  hash_bits < 64 is the bus
        audit's test hook (the grouping key is cut; the report must not change)."""
        opts = _link_opts(max_tuples, max_records_per_tuple, hash_bits)
        return self._audit("link", main, preprocessed, opts)

    def coverage_audit(self, main, preprocessed, deltas=None, max_cells=8192, max_workgroups=0):
        """Which constraint or interaction detects each mutation of the mutation audit (vgpu_coverage_audit): the arguments of prove, deltas as
        in mutation_audit; max_workgroups is a tuning knob (workgroups along a chip's rows, 0: the default) on which the report never depends.
        A CoverageReport back."""
        opts = _coverage_opts(deltas, max_cells, max_workgroups)
        return self._audit("coverage", main, preprocessed, opts)

    def prove_async(self, main, preprocessed, keep=None):
        """Start Machine::prove on a host thread of the library; returns a Ticket (wait() -> Proof).  `keep`: further objects
        (e.g. the operation log the traces were generated from) kept alive until the ticket has been waited for."""
        arr = (ctypes.c_void_p * len(main))(*[t._h for t in main])
        chips = (ctypes.c_uint32 * max(1, len(preprocessed)))(*[c for c, _ in preprocessed])
        parr = (ctypes.c_void_p * max(1, len(preprocessed)))(*[t._h for _, t in preprocessed])
        h = ctypes.c_void_p()
        _check(lib().vgpu_prove_async(self._h, arr, ctypes.c_uint32(len(main)), chips, parr, ctypes.c_uint32(len(preprocessed)), ctypes.byref(h)))
        return Ticket(h, (main, preprocessed, self, keep))

    def set_prep_cache(self, on):
        """Keep the preprocessed commitment across proofs that hand in the same preprocessed traces (off by default: vgpu_prover_set_prep_cache)."""
        lib().vgpu_prover_set_prep_cache(self._h, ctypes.c_uint32(1 if on else 0))

    def set_profiling(self, on, only=None):
        """Per-kernel HIP-event timing on / off (resets the accumulators); only = time launches of this kernel name alone."""
        lib().vgpu_prover_set_profiling_filter(self._h, only.encode() if only else None)
        lib().vgpu_prover_set_profiling(self._h, ctypes.c_uint32(1 if on else 0))

    def profile(self):
        """{kernel: (launches, total_ms, algorithmic_bytes, algorithmic_valu_ops)} accumulated since set_profiling(True)."""
        n = lib().vgpu_prover_profile(self._h, None, ctypes.c_uint64(0))
        buf = ctypes.create_string_buffer(int(n) + 16)
        lib().vgpu_prover_profile(self._h, buf, ctypes.c_uint64(int(n) + 16))
        out = {}
        for line in buf.value.decode().splitlines():
            name, launches, ms, nbytes, ops = line.split()
            out[name] = (int(launches), float(ms), float(nbytes), float(ops))
        return out

    def trim(self):
        """Give the pool's cached free blocks back to the driver; returns the bytes freed."""
        lib().vgpu_prover_trim.restype = ctypes.c_uint64
        return int(lib().vgpu_prover_trim(self._h))

    def reset_memory_peak(self):
        """The pool's peak restarts from what is held now (vgpu_prover_memory_reset_peak)."""
        lib().vgpu_prover_memory_reset_peak(self._h)

    def memory(self):
        live, peak = ctypes.c_uint64(), ctypes.c_uint64()
        lib().vgpu_prover_memory(self._h, ctypes.byref(live), ctypes.byref(peak))
        return live.value, peak.value

    def set_pool_poison(self, word=None, on_alloc=True, on_release=True):
        """Test hook (vgpu_prover_set_pool_poison): fill every block the HBM pool hands out (on_alloc) and every block that returns to its cache
        (on_release) with `word`, synchronously; word None = off.  Refused (VgpuError, code -1) while a proof or an audit owns the context."""
        mode = 0 if word is None else (1 if on_alloc else 0) | (2 if on_release else 0)
        _check(lib().vgpu_prover_set_pool_poison(self._h, ctypes.c_uint32(mode), ctypes.c_uint32(0 if word is None else int(word))))

    def pool_poison_stats(self):
        """(blocks, bytes filled on allocation, blocks, bytes filled on release) since this context was created."""
        out = (ctypes.c_uint64 * 4)()
        lib().vgpu_prover_pool_poison_stats(self._h, out)
        return tuple(int(x) for x in out)

    def pool_peek(self, nbytes, n_words):
        """Test hook (vgpu_prover_pool_peek): take a block of nbytes from the pool as a stage would, read it before writing it, release it.
        Returns (its first n_words words, the last word of the rounded block)."""
        out = np.zeros(int(n_words) + 1, dtype=np.uint32)
        _check(lib().vgpu_prover_pool_peek(self._h, ctypes.c_uint64(int(nbytes)), out.ctypes.data_as(c_u32p), ctypes.c_uint64(int(n_words))))
        return out[:-1].copy(), int(out[-1])

    def lane_stats(self):
        """(trees of this context that entered the device's dense lane, those that waited for another context's event)."""
        entered, waited = ctypes.c_uint64(), ctypes.c_uint64()
        lib().vgpu_prover_lane_stats(self._h, ctypes.byref(entered), ctypes.byref(waited))
        return int(entered.value), int(waited.value)

    def __del__(self):
        if getattr(self, "_h", None):
            try:
                lib().vgpu_prover_destroy(self._h)
            except TypeError:  # interpreter shutdown: module globals already cleared
                pass
            self._h = None
