"""Hand-built batches for the forwarding tests (test infrastructure).

`Source` holds the packets of a one-room configs[0] trace (their VP8
descriptors, payloads and arena stay real); a test picks, reorders or rewrites
them and wraps the result in a `HandTrace`, which is what
tests/test_parity_gpu.py::run_parity reads of a workload.Trace.  The ops a
hand-built case needs go through run_parity's extra_ops.
"""
import ctypes as C

import numpy as np

VIDEO, AUDIO = 0, 1          # the trace's two tracks (configs[0]: one publisher)
T0 = 1700000000 * 10**9


class _NoEvents:
    """Stands in for the generator library: a hand-built trace scripts no ops
    (the tests pass theirs as run_parity's extra_ops)."""

    def lkfs_batch_events(self, h, b, ev, n):
        return 0


class HandTrace:
    """What run_parity reads of a workload.Trace, over hand-built batches:
    `tracks` of the source trace with `ndts` DownTracks each, `batches` a list
    of lists of abi.lkf_pkt (grouped by track; arena_off into `arena`)."""

    def __init__(self, abi, src, tracks, ndts, batches, arena):
        self.src = src  # (keeps the generator's arrays alive)
        self.lib, self.h = _NoEvents(), None
        self.tracks = [abi.lkf_track_params.from_buffer_copy(src.tracks[t]) for t in tracks]
        self.ntracks = len(tracks)
        self.downtracks = []
        for i, t in enumerate(tracks):
            mine = [d for d in range(src.ndts) if src.downtracks[d].track == t][:ndts]
            assert len(mine) == ndts
            for d in mine:
                p = abi.lkf_downtrack_params.from_buffer_copy(src.downtracks[d])
                p.track = i
                self.downtracks.append(p)
        self.ndts = len(self.downtracks)
        self.arena = arena
        self.batches = []
        for pk in batches:
            arr = (abi.lkf_pkt * max(1, len(pk)))()
            for i, p in enumerate(pk):
                arr[i] = p
                arr[i].track = tracks.index(p.track)
            self.batches.append((arr, len(pk)))
        self.nbatches = len(batches)
        m = max(len(pk) for pk in batches)
        self.max_batch_pkts = m
        self.max_batch_arena = len(arena)
        self.max_batch_tuples = m * ndts
        self.max_batch_out_bytes = m * ndts * 1600

    def batch(self, b):
        arr, n = self.batches[b]
        return arr, n, C.cast(self.arena, C.POINTER(C.c_uint8)), len(self.arena)

    def has_dd(self):
        return False


class Source:
    """The packets of a one-room configs[0] trace, per track (and layer), in
    arrival order, over one arena (the batches' arenas back to back)."""

    def __init__(self, workload, abi):
        self.abi = abi
        self.tr = workload.Trace(1, duration_s=4.0, batch_s=1.0)
        assert self.tr.tracks[VIDEO].kind == 1 and self.tr.tracks[AUDIO].kind == 0
        parts, self.pkts, base = [], [], 0
        for b in range(self.tr.nbatches):
            pk, n, ar, alen = self.tr.batch(b)
            parts.append(C.string_at(ar, alen))
            for i in range(n):
                p = abi.lkf_pkt.from_buffer_copy(pk[i])
                p.arena_off += base
                self.pkts.append(p)
            base += alen
        self.arena = C.create_string_buffer(b"".join(parts), base)

    def stream(self, track, layer=None):
        s = [self.abi.lkf_pkt.from_buffer_copy(p) for p in self.pkts
             if p.track == track and (layer is None or p.layer == layer)]
        sn = np.array([p.ext_sn for p in s], dtype=np.int64)
        if layer is not None or track == AUDIO:
            assert (np.diff(sn) == 1).all()  # the source is loss-free and in order: the cases add their own
        return s

    def trace(self, tracks, ndts, batches):
        for b, pk in enumerate(batches):  # arrival: the batch's order, 100 us apart
            for i, p in enumerate(pk):
                p.arrival_ns = T0 + b * 10**9 + i * 100000
        return HandTrace(self.abi, self.tr, tracks, ndts, batches, self.arena)


def start_ops(abi, dts, layer=2):
    """The ops the generator scripts at a video DownTrack's start: the layers
    seen, the maxima and the allocation (target = request = `layer`)."""
    ops = []
    for d in dts:
        ops += [(d, abi.LKF_CTL_SET_MAX_SPATIAL, 2, 0, 0, 0, 0), (d, abi.LKF_CTL_SET_MAX_TEMPORAL, 2, 0, 0, 0, 0),
                (d, abi.LKF_CTL_SET_MAX_SEEN_SPATIAL, 2, 0, 0, 0, 0),
                (d, abi.LKF_CTL_SET_MAX_SEEN_TEMPORAL, 2, 0, 0, 0, 0),
                (d, abi.LKF_CTL_SET_ALLOCATION, layer, 2, layer, 0, 0)]
    return ops
