"""Queues GPU work behind a short bounded stall on the caller's stream, so that the host has finished enqueueing before the
device runs any of it: from the end of the stall on, only the library's event edges order its kernels (a step enqueued
eagerly at these sizes is ordered by the host's launch rate instead, see the head of tests/test_gpu_schedule.py).

    with stalled(S, ms) as st:      # on S: record t0, one sleep kernel of about `ms` milliseconds, record gate
        ...                         # the body: inputs produced by late(), the library calls, clones of the outputs - all on S
    st.premise()                    # `pending`: the gate had not fired when the body was fully enqueued - else the test FAILS
    S.synchronize()                 # the only synchronisation between enqueue and comparison

`run_stalled(S, body, what)` does the whole routine: a warm run of the body (the caching allocator and the library's lazy
attributes settle), one timed run (wall-clock time the host needs to enqueue it), then the run behind a stall of
`stall_ms_for(enqueue ms)` = 4 x that time (the 4 is a margin for host jitter), floored at 20 ms and capped at 250 ms.  It prints a
`[stall]` line with the enqueue time, the stall asked for and the stall achieved.

The stall is ONE `torch.cuda._sleep` kernel whose cycle count comes from `calibrate()` (a sleep of a fixed count timed between
two events); where that kernel does not run, a chain of 4096^2 `torch.mm` calls sized the same way.  Nothing here spins without
a bound.

`stream_gaps(rows)` is pure Python (tests/test_schedule_cpu.py feeds it synthetic timelines): per stream of a timeline, how
much of the span between its first start and last end the stream was busy, and the median gap between one launch's end and
the next one's start.  A timeline led by the device has chain streams that are busy nearly all of their span.

Seen on the MI355X: the sleep kernel ran, 2.394e6 .. 2.395e6 cycles per ms in three processes; a stall asked for 20.0 ms took 19.9 ..
20.0 ms, one of 24.1 ms 24.1 and one of 41.1 ms 41.1.  The host needed 0.34 .. 10.3 ms to enqueue a body (the RA-LENet train pass of
256 windows on four lanes with every kernel kind profiled: 3.7 .. 10.3 ms), so the floor of 20 ms decided all but two stalls;
`pending` was True in all 27 stalled runs.  Per case: the tables in tests/test_gpu_stalled_schedule.py and
tests/test_gpu_stalled_handles.py.
"""
import time

STALL_FLOOR_MS = 20.0
STALL_CAP_MS = 250.0
STALL_MARGIN = 4.0
CAL_CYCLES = 20_000_000
MM_N = 4096


def stall_ms_for(enqueue_ms):
    """the stall for a body the host enqueues in `enqueue_ms`: 4 x, floored at 20 ms, capped at 250 ms"""
    return min(max(STALL_MARGIN * float(enqueue_ms), STALL_FLOOR_MS), STALL_CAP_MS)


def stream_gaps(rows):
    """rows: (kind, stream, t0, t1) in issue order (ms) -> {stream: {"rows", "busy", "median_gap_ms", "max_gap_ms"}}: `busy` is
    the sum of the stream's launch durations over the span from its first start to its last end (1.0 for a single row),
    the gaps are next start minus previous end along the stream's issue order (negative gaps count as 0)."""
    by = {}
    for _, s, t0, t1 in rows:
        by.setdefault(int(s), []).append((float(t0), float(t1)))
    out = {}
    for s, r in by.items():
        span = max(b for _, b in r) - min(a for a, _ in r)
        busy = sum(b - a for a, b in r)
        gaps = sorted(max(n[0] - p[1], 0.0) for p, n in zip(r, r[1:]))
        med = 0.0 if not gaps else (gaps[len(gaps) // 2] if len(gaps) % 2 else 0.5 * (gaps[len(gaps) // 2 - 1] + gaps[len(gaps) // 2]))
        out[s] = {"rows": len(r), "busy": min(busy / span, 1.0) if span > 0 else 1.0, "median_gap_ms": med,
                  "max_gap_ms": gaps[-1] if gaps else 0.0}
    return out


def check_premise(pending, ms, what=""):
    """the premise of every stalled test: the body was fully enqueued while the device was still in the stall.  Anything but
    True fails the test (it never passes or skips on a broken premise)."""
    assert pending is True, (f"premise failed{' (' + what + ')' if what else ''}: the stall of {ms:.1f} ms had ended before the host "
                             "finished enqueueing the body - some call synchronised, or the host was slower than the margin")


def least_busy(rows, streams):
    """the smallest `busy` over the given streams of a timeline (1.0 if none of them has rows)"""
    g = stream_gaps(rows)
    return min([g[s]["busy"] for s in streams if s in g] or [1.0])


# ---------------------------------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------------------------------
_CAL = {}


def _timed(stream, fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        a.record(stream)
        fn()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def calibrate():
    """-> sleep cycles per millisecond (cached): one `torch.cuda._sleep` of CAL_CYCLES timed between two events, after a warm one.
    If the sleep kernel does not run, the stall is a chain of MM_N^2 matrix products and this returns products per millisecond."""
    import torch
    if "per_ms" in _CAL:
        return _CAL["per_ms"]
    s = torch.cuda.Stream()
    try:
        _timed(s, lambda: torch.cuda._sleep(CAL_CYCLES // 100))
        ms = _timed(s, lambda: torch.cuda._sleep(CAL_CYCLES))
        if not ms > 0.0:
            raise RuntimeError("the sleep kernel took no time")
        _CAL.update(kind="sleep", per_ms=CAL_CYCLES / ms)
    except (AttributeError, RuntimeError):
        with torch.cuda.stream(s):
            a = torch.ones(MM_N, MM_N, device="cuda") * (1.0 / MM_N)
            _CAL["mm"] = (a, a.clone(), torch.empty_like(a))

        def chain(n):
            for _ in range(n):
                torch.mm(_CAL["mm"][0], _CAL["mm"][1], out=_CAL["mm"][2])
        _timed(s, lambda: chain(2))
        _CAL.update(kind="mm", per_ms=16 / _timed(s, lambda: chain(16)))
    print(f"[stall] calibration: {_CAL['kind']} stall, {_CAL['per_ms']:.4g} {'cycles' if _CAL['kind'] == 'sleep' else 'products'} per ms")
    return _CAL["per_ms"]


def _enqueue_stall(ms):
    """about `ms` milliseconds of bounded work on the current stream"""
    import torch
    per_ms = calibrate()
    if _CAL["kind"] == "sleep":
        torch.cuda._sleep(int(ms * per_ms))
    else:
        for _ in range(max(int(ms * per_ms + 0.5), 1)):
            torch.mm(_CAL["mm"][0], _CAL["mm"][1], out=_CAL["mm"][2])


class stalled:
    """context manager: on `stream` record t0, enqueue a stall of about `ms` milliseconds, record `gate`; on exit `pending = not
    gate.query()` BEFORE any synchronisation (True: the body was fully enqueued while the device was still in the stall), then
    record t1.  Makes `stream` the current stream inside the block."""

    def __init__(self, stream, ms):
        import torch
        self.stream, self.ms = stream, float(ms)
        self.t0, self.gate, self.t1 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
        self.pending = None
        self._ctx = torch.cuda.stream(stream)

    def __enter__(self):
        calibrate()                                  # (never inside the stall: it synchronises)
        self._ctx.__enter__()
        self.t0.record(self.stream)
        _enqueue_stall(self.ms)
        self.gate.record(self.stream)
        return self

    def __exit__(self, *exc):
        self.pending = not self.gate.query()
        self.t1.record(self.stream)
        self._ctx.__exit__(*exc)
        return False

    def premise(self, what=""):
        check_premise(self.pending, self.ms, what)

    def achieved_ms(self):
        """t0 -> gate on the device (call after the stream has been synchronised)"""
        return self.t0.elapsed_time(self.gate)

    def body_ms(self):
        """gate -> t1 on the device: what the body took once the stall let it go"""
        return self.gate.elapsed_time(self.t1)


def poison(t):
    """NaN into a floating-point tensor, a fixed wrong value into an integer one (on the current stream)"""
    if t.is_floating_point():
        t.fill_(float("nan"))
    else:
        t.fill_(-12345 if t.dtype.is_signed else 123)
    return t


def late(dst, src):
    """dst.copy_(src) on the current stream: behind a stall, `dst` holds its value only for work that is ordered after it"""
    dst.copy_(src)
    return dst


def run_stalled(stream, body, what, before=None):
    """warm run, timed run, stalled run of `body()` on `stream`; `before()` runs on `stream` in front of each (poisoning the buffers
    the body fills) and is waited for.  -> (the stalled run's return value, the `stalled` object, host enqueue ms).  The premise
    is asserted; on return `stream` has been synchronised - nothing else has."""
    import torch
    calibrate()

    def prepare():
        with torch.cuda.stream(stream):
            if before is not None:
                before()
        stream.synchronize()

    prepare()
    with torch.cuda.stream(stream):
        body()
    stream.synchronize()
    prepare()
    with torch.cuda.stream(stream):
        h0 = time.perf_counter()
        body()
        enqueue_ms = (time.perf_counter() - h0) * 1e3
    stream.synchronize()
    prepare()
    with stalled(stream, stall_ms_for(enqueue_ms)) as st:
        out = body()
    stream.synchronize()
    print(f"[stall] {what}: host enqueue {enqueue_ms:.2f} ms, stall asked {st.ms:.1f} ms, achieved {st.achieved_ms():.1f} ms, "
          f"body behind it {st.body_ms():.2f} ms, pending {st.pending}")
    st.premise(what)
    return out, st, enqueue_ms
