"""A gate for the stream-contract tests (tests/test_gpu_stream_order.py) and the table that classifies every entry point of
include/psfm.h that takes `void* stream` (tests/test_stream_contract_table.py checks it on the CPU).

The gate: on a side stream that does not synchronise with the null stream, a device delay (torch.cuda._sleep, calibrated to
DELAY_MS with events; a fixed chain of matmuls where _sleep is missing or does nothing) followed by copies of the REAL inputs over
buffers that until then hold a DECOY -- a valid input of the same shape whose correct result differs.  Work that the library
enqueues on the caller's stream runs behind the copies and sees the real input; work that it puts on any other stream (the null
stream, torch's current stream, an internal stream without an event edge) runs at once, reads the decoy and gives wrong bytes --
never an out-of-range access.  The delay is a bounded spin: nothing here waits on a device flag.

What the gate can and cannot show.  A process has a few hardware queues (four by default) and the runtime spreads its streams over
them; two streams on one queue run in order whether or not an event joins them.  Gate() therefore takes the first pair of fresh
streams (of at most six pairs; torch hands them out of its own pool and keeps them, nothing is created per attempt that could be
released) that the null stream and a second stream really overtake, and fails the module when no pair does.  The same sharing means
that a stream INSIDE the library (psfm_connect's side stream, the copy streams of psfm_load_flo_stack, the redo stream of
psfm_connect_batch) may sit on the gated stream's queue, where a missing event edge stays hidden: for work the library moves to a
stream of its own -- classes (c), (d), (e) of tests/test_gpu_stream_order.py -- a pass is evidence, not proof, and detection is
probabilistic; a launch on the null stream or on torch's current stream is always caught (the self-check proves both overtake).

The validity condition: finish() asserts that the host was done enqueueing (enqueued(), called where the last asynchronous call
has returned, or at the ENTRY of the first synchronising call) within half the delay and while the gate still held."""
import contextlib
import ctypes
import time

import numpy as np

DELAY_MS = 50.0
HIP_STREAM_NON_BLOCKING = 0x01

# ---------------------------------------------------------------------------------------------------------------------------------
# Every exported function of include/psfm.h that takes `void* stream`, by what the header promises about that stream:
#   "async"          work is enqueued on `stream` and the call returns without synchronising the host
#   "synchronising"  work is enqueued on `stream` (or ordered behind it) and the call synchronises it before it returns
#   ("exempt", why)  not exercised by tests/test_gpu_stream_order.py
# A new entry point cannot be added to the header without a row here (tests/test_stream_contract_table.py).
_SHARD = "one step of the sharded engine: needs the whole protocol (several ranks); tests/test_gpu_sharded.py drives it on side streams"
STREAM_CONTRACT = {
    "psfm_motion_boundary": "async",
    "psfm_kill_map": "async",
    "psfm_kill_map_batch": "async",
    "psfm_flow_check": "async",
    "psfm_grid_sample": "async",
    "psfm_path_consistency_eval": "async",
    "psfm_sort_records": "async",
    "psfm_sort_records64": "async",
    "psfm_traj_augment": "async",
    "psfm_traj_encode": "async",
    "psfm_traj_decode": "async",
    "psfm_traj_decode_batch": "async",
    "psfm_window_sample_batch": "async",            # its FILL form; the PLAN form synchronises once and is made beforehand
    "psfm_traj_augment_batch": "async",
    "psfm_traj_encode_batch": "async",
    "psfm_labels_begin": "async",
    "psfm_labels_merge_window": "async",
    "psfm_traj_eval_counts": "async",
    "psfm_load_flo_stack": "synchronising",
    "psfm_track": "synchronising",
    "psfm_connect": "synchronising",
    "psfm_connect_batch": "synchronising",
    "psfm_result_copy": "synchronising",
    "psfm_result_filter": "synchronising",
    "psfm_result_filtered_copy": "synchronising",
    "psfm_window_sample": "synchronising",
    "psfm_traj_to_matches": "synchronising",
    "psfm_matches_copy": "synchronising",
    "psfm_labels_finish": "synchronising",
    "psfm_labels_copy": "synchronising",
    "psfm_labels_to_matches": "synchronising",
    "psfm_matches_to_database": "synchronising",
    "psfm_database_copy": "synchronising",
    "psfm_track_queries": "synchronising",
    "psfm_track_queries_optimize": "synchronising",
    "psfm_optimize_location": "synchronising",
    "psfm_track_queries_batch": "synchronising",
    "psfm_track_queries_optimize_batch": "synchronising",
    "psfm_result_filter_batch": "synchronising",
    "psfm_traj_to_matches_batch": "synchronising",
    "psfm_labels_to_matches_batch": "synchronising",
    "psfm_labels_set": "synchronising",
    "psfm_database_compact_again": ("exempt", "a measurement hook that repeats one launch of psfm_matches_to_database, which is gated"),
    "psfm_sparse_depth": "synchronising",
    "psfm_sparse_depth_sort_ids": "synchronising",
    "psfm_depth_display": "synchronising",
    "psfm_traj_vote_labels": "synchronising",
    "psfm_result_keys": ("exempt", "the id keys of the sharded engine; tests/test_gpu_sharded.py reads them on side streams"),
    "psfm_shard_begin": ("exempt", _SHARD),
    "psfm_shard_step": ("exempt", _SHARD),
    "psfm_shard_solve_export": ("exempt", _SHARD),
    "psfm_shard_frame": ("exempt", _SHARD),
    "psfm_shard_solve_control": ("exempt", _SHARD),
    "psfm_shard_solve_control_async": ("exempt", _SHARD),
    "psfm_shard_window_state": ("exempt", _SHARD),
    "psfm_shard_solve_control_chain_async": ("exempt", _SHARD),
    "psfm_shard_solve_poll": ("exempt", _SHARD),
    "psfm_shard_solve_local": ("exempt", _SHARD),
    "psfm_shard_solve_redo_local": ("exempt", _SHARD),
    "psfm_shard_peer_area": ("exempt", _SHARD),
    "psfm_shard_peer_epoch": ("exempt", _SHARD),
    "psfm_shard_solve_peer": ("exempt", _SHARD),
    "psfm_shard_solve_restore": ("exempt", _SHARD),
    "psfm_shard_solve_writeback": ("exempt", _SHARD),
    "psfm_shard_finish": ("exempt", _SHARD),
}


def contract_class(name):
    c = STREAM_CONTRACT[name]
    return c if isinstance(c, str) else c[0]


# ---------------------------------------------------------------------------------------------------------------------------------
_runtime = []


def _hip_runtime():
    """The HIP runtime that is already in the process (torch's), through ctypes; looked up once."""
    if _runtime:
        return _runtime[0]
    path = None
    with open("/proc/self/maps") as fp:
        for line in fp:
            if "libamdhip64" in line:
                path = line.split()[-1]
                break
    assert path is not None, "no HIP runtime is loaded: import torch and touch the device first"
    rt = ctypes.CDLL(path)
    rt.hipStreamGetFlags.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint)]
    rt.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    _runtime.append(rt)
    return rt


def stream_flags(stream):
    flags = ctypes.c_uint(0xFFFFFFFF)
    err = _hip_runtime().hipStreamGetFlags(ctypes.c_void_p(stream.cuda_stream), ctypes.byref(flags))
    assert err == 0, "hipStreamGetFlags failed with %d" % err
    return int(flags.value)


def non_blocking_stream():
    """A stream that does not synchronise with the null stream: torch's own where it is one, else one made for the purpose."""
    import torch
    s = torch.cuda.Stream()
    flags = stream_flags(s)
    if flags & HIP_STREAM_NON_BLOCKING:
        return s, flags
    raw = ctypes.c_void_p()
    err = _hip_runtime().hipStreamCreateWithFlags(ctypes.byref(raw), HIP_STREAM_NON_BLOCKING)
    assert err == 0 and raw.value, "hipStreamCreateWithFlags failed with %d" % err
    s = torch.cuda.ExternalStream(raw.value)
    return s, stream_flags(s)


class Gate:
    """One per test module (gate()).  close(pairs) enqueues the delay and the copies dst <- src on the side stream; finish(what)
    synchronises it and asserts that everything was enqueued while the gate still held."""

    def __init__(self):
        import torch
        self.torch = torch
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        torch.cuda.synchronize()
        self._matmul = None
        self._calibrate()
        self.side = self.observer = None
        tried = []
        for attempt in range(6):        # streams share a few hardware queues: take a side stream that the null stream and a second
            side, flags = non_blocking_stream()         # stream can really overtake
            observer, oflags = non_blocking_stream()
            assert flags & HIP_STREAM_NON_BLOCKING and oflags & HIP_STREAM_NON_BLOCKING, (flags, oflags)
            seen = self._self_check(side, observer)
            tried.append(seen)
            print("stream gate: side stream %#x flags %#x, observer %#x flags %#x: unordered copy saw %s, null-stream copy saw %s, "
                  "ordered copy saw %s" % (side.cuda_stream, flags, observer.cuda_stream, oflags, seen[0], seen[1], seen[2]))
            if seen == ("the decoy", "the decoy", "the real bytes"):
                self.side, self.observer, self.flags = side, observer, flags
                break
            assert seen[2] == "the real bytes", "a copy enqueued behind the gate on its own stream did not see the real bytes"
        assert self.side is not None, ("the gate does not work: a copy with no event edge to the gated stream saw the real bytes "
                                       "on every stream tried (%r)" % (tried,))
        self.ptr = ctypes.c_void_p(self.side.cuda_stream)
        self._t0 = self._t1 = None

    # -- the delay --
    def _delay(self):
        if self._matmul is None:
            self.torch.cuda._sleep(self.cycles)
        else:
            a = self._matmul
            for _ in range(self.cycles):
                a = (a @ self._matmul) * 0.5

    def _measure(self):
        torch = self.torch
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s):
            e0.record()
            self._delay()
            e1.record()
        s.synchronize()
        return float(e0.elapsed_time(e1))

    def _calibrate(self):
        torch = self.torch
        ms = 0.0
        if hasattr(torch.cuda, "_sleep"):
            self.cycles = 2_000_000
            self._measure()
            ms = self._measure()
        if ms < 0.05:                   # missing, or a no-op on this device: a fixed chain of matmuls
            self._matmul = torch.full((1024, 1024), 1.0 / 1024, dtype=torch.float32, device="cuda")
            self.cycles = 64
            self._measure()
            ms = self._measure()
        self.cycles = max(int(self.cycles * DELAY_MS / ms), 1)
        self.delay_ms = min(self._measure(), self._measure())
        print("stream gate: delay of %d %s calibrated to %.1f ms (target %.0f ms)"
              % (self.cycles, "matmuls" if self._matmul is not None else "_sleep cycles", self.delay_ms, DELAY_MS))
        assert 0.6 * DELAY_MS <= self.delay_ms <= 4 * DELAY_MS, "the delay could not be calibrated"

    # -- the self-check --
    def _self_check(self, side, observer):
        torch = self.torch
        decoy = torch.full((1 << 16,), 0x11, dtype=torch.uint8, device="cuda")
        real = torch.full((1 << 16,), 0xEE, dtype=torch.uint8, device="cuda")
        buf = decoy.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            self._delay()
            buf.copy_(real)
        with torch.cuda.stream(observer):
            unordered = buf.clone()
        on_null = buf.clone()
        with torch.cuda.stream(side):
            ordered = buf.clone()
        torch.cuda.synchronize()
        name = lambda t: "the decoy" if torch.equal(t, decoy) else "the real bytes" if torch.equal(t, real) else "a mixture"
        return name(unordered), name(on_null), name(ordered)

    # -- use --
    def on_side(self):
        return self.torch.cuda.stream(self.side)

    def close(self, pairs):
        """Everything enqueued so far is completed first; then, on the side stream: the delay, then dst.copy_(src) for every pair."""
        self.torch.cuda.synchronize()
        with self.on_side():
            self._delay()
            for dst, src in pairs:
                dst.copy_(src)
        self._t0 = time.perf_counter()
        self._t1 = None

    def holds(self):
        """True while the gate (or anything behind it on the side stream) has not completed."""
        return not self.side.query()

    def enqueued(self):
        """Marks the end of the host's enqueueing (finish() does it otherwise): the first mark behind close() counts."""
        if self._t1 is None:
            self._t1 = time.perf_counter()
            self._held = self.holds()

    def finish(self, what):
        if self._t1 is None:
            self.enqueued()
        self.side.synchronize()
        self.torch.cuda.synchronize()
        ms = (self._t1 - self._t0) * 1e3
        print("%s: enqueued in %.2f ms behind a gate of %.1f ms%s" % (what, ms, self.delay_ms, "; the gate still held then" if self._held else "; THE GATE HAD OPENED by then"))
        assert self._held, "INVALID, not passed: the gate had opened before everything was enqueued (%s)" % what
        assert ms < 0.5 * self.delay_ms, ("INVALID, not passed: the host took %.2f ms to enqueue, the gate holds %.1f ms -- it may have "
                                          "expired before the calls were queued" % (ms, self.delay_ms))


_gate = None


def gate():
    global _gate
    if _gate is None:
        _gate = Gate()
    return _gate


# ---------------------------------------------------------------------------------------------------------------------------------
GUARD = 4096            # bytes behind every output that must come back untouched


class Buf:
    """One device buffer of a call.  role "in": real / decoy host arrays, gated; "inout": the same, and snapshotted (in-place calls);
    "out": `nbytes` of sentinel bytes and a guard behind them, snapshotted; "ws": a caller-owned workspace whose contents may be
    anything (filled with `fill` before, 0xFF behind the call) and a guard behind it; "const": uploaded once (weights)."""

    def __init__(self, role, real=None, decoy=None, nbytes=0, fill=0xA5):
        import torch
        self.role, self.fill = role, fill
        if role in ("in", "inout", "const"):
            real = np.ascontiguousarray(real)
            self.real = torch.from_numpy(real.view(np.uint8).reshape(-1).copy()).cuda()
            self.nbytes = int(self.real.numel())
            if role != "const":
                decoy = np.ascontiguousarray(decoy)
                assert decoy.dtype == real.dtype and decoy.shape == real.shape, "a decoy has the shape and type of the real input"
                self.decoy = torch.from_numpy(decoy.view(np.uint8).reshape(-1).copy()).cuda()
            guard = GUARD if role == "inout" else 0
            self.t = torch.full((self.nbytes + guard + 16,), 0x5A, dtype=torch.uint8, device="cuda")
            if role == "const":
                self.t[:self.nbytes] = self.real
        else:
            self.nbytes = int(nbytes)
            self.t = torch.full((self.nbytes + GUARD,), fill, dtype=torch.uint8, device="cuda")
            self.t[self.nbytes:] = 0x5A
            self.blank = torch.full((self.nbytes,), fill, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def load(self, which):
        self.t[:self.nbytes] = self.real if which == "real" else self.decoy

    def reset(self):
        self.t[:self.nbytes] = self.fill

    def host(self, dtype=np.uint8, shape=None):
        a = self.t[:self.nbytes].cpu().numpy().view(dtype)
        return a if shape is None else a.reshape(shape)


def IN(real, decoy):
    return Buf("in", real, decoy)


def INOUT(real, decoy):
    return Buf("inout", real, decoy)


def CONST(real):
    return Buf("const", real)


def OUT(nbytes, fill=0xA5):
    return Buf("out", nbytes=nbytes, fill=fill)


def WS(nbytes, fill=0xA5):
    return Buf("ws", nbytes=nbytes, fill=fill)


class Call:
    """One call of an entry point: bufs {name: Buf}, fn(stream_ptr, bufs) -> status, check(outs) against the suite's reference of
    the operation, outs = {name: uint8 host array of the output's bytes}."""

    def __init__(self, name, bufs, fn, check=None, min_differ=16):
        self.name, self.bufs, self.fn, self.check, self.min_differ = name, bufs, fn, check, min_differ

    def roles(self, *roles):
        return [(n, b) for n, b in self.bufs.items() if b.role in roles]

    def _default_stream_run(self, which):
        import torch
        for _, b in self.roles("in", "inout"):
            b.load(which)
        for _, b in self.roles("out", "ws"):
            b.reset()
        torch.cuda.synchronize()
        st = self.fn(ctypes.c_void_p(0), self.bufs)
        assert st == 0, "%s: status %d on the default stream" % (self.name, st)
        torch.cuda.synchronize()
        return {n: b.t.cpu().numpy().copy() for n, b in self.roles("out", "inout")}

    def expected(self):
        """The call on the default stream with full synchronisation: on the decoy, then on the real input (which also warms the
        context's scratch).  The two results must differ in many bytes; the real one is checked against the reference."""
        dec = self._default_stream_run("decoy")
        self.want = self._default_stream_run("real")
        differ = sum(int((dec[n] != self.want[n]).sum()) for n in self.want)
        print("%s: the decoy's result differs from the real input's in %d bytes" % (self.name, differ))
        assert differ >= self.min_differ, "%s: the decoy does not tell a read that ran too early" % self.name
        if self.check is not None:
            self.check({n: self.want[n][:self.bufs[n].nbytes] for n in self.want})
        return self.want


def run_gated(calls, what, asynchronous=True, order=None):
    """calls: one Call, or several queued back to back behind ONE gate.  The sequence of the issue's (a) / (b): expected bytes from
    the default stream (`order`: the order of those warming runs, default as given), the inputs hold the decoy, the gate, the calls on
    the side stream (its pointer passed explicitly, torch's current stream stays the default one), `not query()` for asynchronous
    calls, a snapshot of the outputs behind each call, the inputs overwritten with the decoy and the workspaces with 0xFF behind
    them all, one synchronisation; every snapshot equals its own expected bytes, guards included."""
    import torch
    g = gate()
    calls = calls if isinstance(calls, (list, tuple)) else [calls]
    for c in (order or calls):
        c.expected()
    pairs = []
    for c in calls:
        for _, b in c.roles("in", "inout"):
            b.load("decoy")
            pairs.append((b.t[:b.nbytes], b.real))
        for _, b in c.roles("out", "ws"):
            b.reset()
        for _, b in c.roles("out"):         # the gate also blanks the outputs: a launch that ran ahead of it is wiped out
            pairs.append((b.t[:b.nbytes], b.blank))
    assert torch.cuda.current_stream().cuda_stream == 0, "torch's current stream is the default stream in these tests"
    g.close(pairs)
    status, held, snaps = [], [], []
    for c in calls:
        status.append(c.fn(g.ptr, c.bufs))
        held.append(g.holds())
        with g.on_side():
            snaps.append({n: b.t.clone() for n, b in c.roles("out", "inout")})
    with g.on_side():
        for c in calls:
            for _, b in c.roles("in"):
                b.load("decoy")
            for _, b in c.roles("ws"):
                b.t[:b.nbytes] = 0xFF
    g.finish(what)
    assert all(st == 0 for st in status), (what, status)
    if asynchronous:
        assert all(held), "%s: the call returned only after the gate had opened -- it synchronised the host (%r)" % (what, held)
    for c, snap in zip(calls, snaps):
        for n, t in snap.items():
            got = t.cpu().numpy()
            bad = int((got != c.want[n]).sum())
            assert bad == 0, ("%s: %s of %s behind the gate differs from the default-stream run in %d bytes (%d of them in the guard)"
                              % (what, n, c.name, bad, int((got[c.bufs[n].nbytes:] != c.want[n][c.bufs[n].nbytes:]).sum())))
        for n, b in c.roles("ws", "out", "inout"):
            tail = b.t[b.nbytes:b.nbytes + GUARD].cpu().numpy()
            assert (tail == 0x5A).all(), "%s: wrote behind %s" % (what, n)


@contextlib.contextmanager
def gated_inputs(pairs, what):
    """For synchronising entry points: `pairs` = [(device buffer that holds the decoy, device tensor with the real bytes)].  Inside
    the block the gate is closed; the caller makes its calls with gate().ptr and marks the ENTRY of the first one with
    g.enqueued() (a synchronising call returns only when the gate has opened): the time up to there, and the gate still holding
    there, are what finish() asserts."""
    g = gate()
    g.close(pairs)
    assert g.holds()
    yield g
    g.finish(what)
