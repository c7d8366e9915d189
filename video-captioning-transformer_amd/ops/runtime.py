"""The host runtime (csrc/vct_runtime.hip): cross-stream ordering, recorded launch lists and the live timing of tagged
launches (bench.py roofline) -- HIP event pairs recorded by the C runtime on the launch stream, so they also fire inside
replayed launch lists.  The tap state and the recording of this thread live here and nowhere else."""
import threading

import torch

from .. import _lib as L
from ._common import _sptr


def stream_wait(waiter, signal):
    """`waiter` (torch stream, None = current) waits for everything enqueued so far on `signal`.  Recordable."""
    L.check(L.load().vct_stream_wait(_sptr(waiter), _sptr(signal)), "vct_stream_wait")


def sync_record(ident: int, stream=None):
    L.check(L.load().vct_sync_record(int(ident), _sptr(stream)), "vct_sync_record")


def sync_wait(ident: int, stream=None):
    L.check(L.load().vct_sync_wait(int(ident), _sptr(stream)), "vct_sync_wait")


_rec = threading.local()     # .ll = the LaunchList recording on THIS thread (the C recorder is thread_local too): host-side collectives
                             # issued on another thread while this one records run immediately, as they must


def is_recording() -> bool:
    return getattr(_rec, "ll", None) is not None


def host_call(fn, stream=None):
    """Run the Python callable `fn()` on the host once everything enqueued on `stream` (None = current) so far has finished --
    immediately, or at this point of every replay while a launch list records (include/vct_hip.h, vct_cmdlist_host_call).  For
    host-side collectives (torch.distributed / gloo) inside a recorded step; an exception in fn becomes status 1 of the replay."""
    def thunk(_arg):
        try:
            fn()
            return 0
        except Exception:                     # never unwind through the C frames of the replay loop
            import traceback
            traceback.print_exc()
            return 1
    cfn = L.HOST_FN(thunk)
    ll = getattr(_rec, "ll", None)
    if ll is not None:
        ll._thunks.append(cfn)            # the recording owns its thunks (and the tensors they capture): released with the list
    L.check(L.load().vct_cmdlist_host_call(L.C.cast(cfn, L.vp), None, _sptr(stream)), "vct_cmdlist_host_call")


def masked_stream(cu_bits, device=None):
    """torch stream restricted to the compute units whose indices are in `cu_bits` (iterable of ints < 256); an empty /
    None selection gives an ordinary stream.  Wraps vct_stream_create_masked; the stream lives as long as the process."""
    words = (L.u32 * 8)()
    n = 0
    for c in (cu_bits or ()):
        words[c // 32] |= (1 << (c % 32))
        n += 1
    h = L.vp()
    L.check(L.load().vct_stream_create_masked(words, 8 if n else 0, L.C.byref(h)), "vct_stream_create_masked")
    return torch.cuda.ExternalStream(h.value, device=device)


TAPS = {"gen_fwd": 0, "gen_dx": 1, "gen_dw": 2, "layers_fwd": 3, "loss": 4, "adam": 5, "step": 6,
        # data-parallel exchange (trainer.ShardedExchange): what the compute stream WAITS for the communicator at the end of a step,
        # and how long each gradient bucket (reduce-scatter -> Adam on the shard -> all-gather -> cast) occupies the communicator's stream
        "comm_wait": 7, **{f"comm_b{i}": 8 + i for i in range(8)},
        # the two sample-stationary stack launches of the forward (encoder incl. its front end / decoder incl. the token embedding)
        "ss_enc": 16, "ss_dec": 17}
_taps_on = False
_taps_only = None        # None = every tag, else the set of tags that are bracketed


def taps_enable(on: bool, only=None):
    """Switch the live timing brackets on / off; `only`: an iterable of tags to restrict them to.  Every bracket is two HIP event
    records in the step's stream -- seven brackets cost the cfg-B step ~55 us (tools/taps_cost.py) -- so a benchmark keeps only the
    one it needs inside its timed region.  Recorded launch lists / graphs contain the brackets that were active when they were
    made: drop them (CaptionTrainer.drop_recordings) after changing this."""
    global _taps_on, _taps_only
    _taps_on = bool(on)
    _taps_only = None if only is None else frozenset(only)
    L.check(L.load().vct_tap_enable(int(_taps_on)), "vct_tap_enable")


def tap_active(tag: str) -> bool:
    """Whether brackets of `tag` are recorded now; while taps are disabled this is one boolean test."""
    return _taps_on and (_taps_only is None or tag in _taps_only)


def tap(tag: str, phase: int, stream=None):
    """Bracket a region of `stream` with HIP timing events (phase 0 = start, 1 = end); no-op while taps are disabled."""
    if tap_active(tag):
        L.check(L.load().vct_tap(TAPS[tag], phase, _sptr(stream)), "vct_tap")


def tap_collect(tag: str, cap: int = 4096):
    """Elapsed milliseconds of every bracket of `tag` executed since the last collect (waits for them)."""
    buf = (L.f32 * cap)()
    n = L.load().vct_tap_collect(TAPS[tag], buf, cap)
    if n < 0:
        L.check(n, "vct_tap_collect")
    return [float(buf[i]) for i in range(n)]


class LaunchList:
    """One recorded step: `with ll.record(): <issue the step>` captures every vct_* launch made on this thread (nothing
    executes), `ll.replay()` re-issues them from C.  Launches aimed at the stream that was current at record time go to
    the stream current at replay time."""

    def __init__(self):
        h = L.vp()
        L.check(L.load().vct_cmdlist_create(L.C.byref(h)), "vct_cmdlist_create")
        self._h = h
        self._thunks = []                 # host-call thunks of this recording (ops.host_call)

    class _Rec:
        def __init__(self, ll):
            self.ll = ll

        def __enter__(self):
            L.check(L.load().vct_cmdlist_begin(self.ll._h, L.stream_ptr()), "vct_cmdlist_begin")
            self.ll._thunks = []          # a re-recording replaces the commands, and with them the thunks they call
            _rec.ll = self.ll
            return self.ll

        def __exit__(self, *exc):
            _rec.ll = None
            L.check(L.load().vct_cmdlist_end(self.ll._h), "vct_cmdlist_end")
            return False

    def record(self):
        return LaunchList._Rec(self)

    def replay(self):
        L.check(L.load().vct_cmdlist_replay(self._h, L.stream_ptr()), "vct_cmdlist_replay")

    def __len__(self):
        return int(L.load().vct_cmdlist_size(self._h))

    @property
    def n_streams(self):
        return int(L.load().vct_cmdlist_streams(self._h))

    def close(self):
        if self._h is not None and self._h.value:
            L.load().vct_cmdlist_destroy(self._h)
            self._h = None
            self._thunks = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
