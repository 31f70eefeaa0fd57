"""lkfwd — MI355X-native batched RTP forwarding engine (livekit-server SFU hot path).

The product is ``lib/liblkfwd.so`` (gfx950 HIP kernels + C++ host engine,
C-ABI in ``include/lkfwd.h``).  This module is a thin ctypes loader used by the
tests and bench: it never computes anything itself and has no CPU fallback —
if the HIP library is missing or no GPU is present, it raises.

Import with ``importlib.import_module("livekit-server_amd")`` (the directory
name contains a hyphen).
"""
import ctypes as C
import os

import numpy as np

from . import abi

# LKF_LIB names another build of the engine in lib/ (liblkfwd_checked.so: the
# bounds-checked kernels of `make` target liblkfwd_checked.so)
LIB_PATH = os.path.join(abi.LIBDIR, os.environ.get("LKF_LIB", "liblkfwd.so"))
_lib = None


class EngineError(RuntimeError):
    pass


def load_library(path=None):
    """Loads liblkfwd.so (raises if it has not been built)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError("liblkfwd.so not built (%s): run __graft_entry__.build()" % p)
    lib = C.CDLL(p)
    v = C.c_void_p
    lib.lkf_create.restype = v
    lib.lkf_create.argtypes = [C.c_int, C.POINTER(abi.lkf_cfg)]
    lib.lkf_destroy.restype = None
    lib.lkf_destroy.argtypes = [v]
    lib.lkf_last_error.restype = C.c_char_p
    lib.lkf_last_error.argtypes = [v]
    lib.lkf_version.restype = C.c_char_p
    lib.lkf_version.argtypes = []
    lib.lkf_submit.restype = C.c_int
    lib.lkf_submit.argtypes = [v, v, C.c_uint32, v, C.c_uint64]
    lib.lkf_submit_device.restype = C.c_int
    lib.lkf_submit_device.argtypes = [v, v, C.c_uint32, v, C.c_uint64]
    lib.lkf_run.restype = C.c_int
    lib.lkf_run.argtypes = [v, v]
    lib.lkf_sync.restype = C.c_int
    lib.lkf_sync.argtypes = [v]
    lib.lkf_output_device.restype = C.c_int
    lib.lkf_output_device.argtypes = [v, C.POINTER(v), C.POINTER(C.c_uint64), C.POINTER(v), C.POINTER(C.c_uint64)]
    lib.lkf_last_timings.restype = C.c_int
    lib.lkf_last_timings.argtypes = [v, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.lkf_timing_window.restype = C.c_int
    lib.lkf_timing_window.argtypes = [v, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float),
                                      C.POINTER(C.c_float)]
    lib.lkf_get_cumulative.restype = C.c_int
    lib.lkf_get_cumulative.argtypes = [v, C.POINTER(abi.lkf_stats), C.c_int]
    if hasattr(lib, "lkf_debug_check"):
        lib.lkf_debug_check.restype = C.c_int
        lib.lkf_debug_check.argtypes = [v, C.POINTER(C.c_uint64), C.c_int]
    lib.api = abi.bind_engine_api(lib, "lkf_")
    if path is None:
        _lib = lib
    return lib


def debug_check(reset=True):
    """Bounds-check record of a checked build (LKF_LIB=liblkfwd_checked.so):
    (violations, first site, its index, its capacity), or None for a product
    build."""
    lib = load_library()
    out = (C.c_uint64 * 4)()
    rc = lib.lkf_debug_check(None, out, 1 if reset else 0)
    if rc != 0:
        return None
    return tuple(int(x) for x in out)


def drain_arrays(api, h, nmax=None):
    """Reads the last batch's records + wire bytes into numpy arrays."""
    n = C.c_uint64()
    alen = C.c_uint64()
    rc = api["drain"](h, None, 0, None, 0, C.byref(n), C.byref(alen))
    if rc not in (0, -28):  # -28: ENOSPC for the size probe
        raise EngineError("drain probe rc=%d" % rc)
    recs = np.zeros(n.value, dtype=abi.OUT_DTYPE)
    arena = np.zeros(alen.value, dtype=np.uint8)
    rc = api["drain"](h, recs.ctypes.data, n.value, arena.ctypes.data, alen.value, C.byref(n), C.byref(alen))
    if rc != 0:
        msg = api["last_error"](h).decode() if "last_error" in api else ""
        raise EngineError("drain rc=%d (%d records, %d bytes): %s" % (rc, n.value, alen.value, msg))
    return recs, arena


def transport_params(master_key, master_salt, profile=abi.LKF_SRTP_AES128_CM_HMAC_SHA1_80):
    """lkf_transport_params from a DTLS-SRTP export: 16 key bytes and 14 salt
    bytes (12 for AEAD_AES_128_GCM)."""
    t = abi.lkf_transport_params()
    C.memmove(t.master_key, bytes(master_key), 16)
    C.memmove(t.master_salt, bytes(master_salt), len(master_salt))
    t.profile = profile
    return t


def drain_protected(api, h):
    """The last protected run's arena (record i's packet at out_off + 16 * i)."""
    n = C.c_uint64()
    rc = api["drain_protected"](h, None, 0, C.byref(n))
    if rc not in (0, -28):
        raise EngineError("drain_protected probe rc=%d" % rc)
    arena = np.zeros(n.value, dtype=np.uint8)
    rc = api["drain_protected"](h, arena.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise EngineError("drain_protected rc=%d" % rc)
    return arena


def twcc_words(api, h):
    """Per-datagram TWCC responder push words (LKF_TWCC_*) of the last ingest."""
    n = C.c_uint32()
    rc = api["ingest_twcc"](h, None, 0, C.byref(n))
    if rc not in (0, -28):
        raise EngineError("ingest_twcc probe rc=%d" % rc)
    out = np.zeros(n.value, dtype=np.uint32)
    rc = api["ingest_twcc"](h, out.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise EngineError("ingest_twcc rc=%d" % rc)
    return out


def flows_array(api, h):
    """Per-datagram outcomes (lkf_flow) of the last ingest as a numpy array."""
    n = C.c_uint32()
    rc = api["ingest_flows"](h, None, 0, C.byref(n))
    if rc not in (0, -28):
        raise EngineError("ingest_flows probe rc=%d" % rc)
    out = np.zeros(n.value, dtype=abi.FLOW_DTYPE)
    rc = api["ingest_flows"](h, out.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise EngineError("ingest_flows rc=%d" % rc)
    return out


def nacks_arrays(api, h):
    """lkf_ingest_nacks: the last ingest's RTCP NACKs (RTCP_NACK_DTYPE) and
    their pairs (NACK_PAIR_DTYPE)."""
    n = C.c_uint32()
    npairs = C.c_uint32()
    rc = api["ingest_nacks"](h, None, 0, None, 0, C.byref(n), C.byref(npairs))
    if rc not in (0, -28):
        raise EngineError("ingest_nacks probe rc=%d" % rc)
    recs = np.zeros(n.value, dtype=abi.RTCP_NACK_DTYPE)
    pairs = np.zeros(npairs.value, dtype=abi.NACK_PAIR_DTYPE)
    rc = api["ingest_nacks"](h, recs.ctypes.data, n.value, pairs.ctypes.data, npairs.value, C.byref(n),
                             C.byref(npairs))
    if rc != 0:
        raise EngineError("ingest_nacks rc=%d" % rc)
    return recs, pairs


def speakers_array(api, h, now_ns):
    """Room.GetActiveSpeakers for every room at now_ns as a numpy array."""
    n = C.c_uint32()
    cap = 4096
    while True:
        out = np.zeros(cap, dtype=abi.SPEAKER_DTYPE)
        rc = api["speakers"](h, now_ns, out.ctypes.data, cap, C.byref(n))
        if rc == 0:
            return out[:n.value]
        if rc != -28:
            raise EngineError("speakers rc=%d" % rc)
        cap = n.value


def room_summaries_enqueue(api, h, now_ns, room_ids, spk_ptr, k, bwe_ptr, s, stream_ptr):
    """lkf_room_summaries_enqueue: the speaker and bandwidth records of the
    rooms `room_ids` (ascending) packed into device buffers spk int32
    [rows, k, 3] / bwe int64 [rows, s, 5] on the caller stream `stream_ptr`,
    without a host wait (rooms.pack_speakers / rooms.fold_summaries layout)."""
    ids = np.ascontiguousarray(np.asarray(room_ids, dtype=np.uint32))
    rc = api["room_summaries_enqueue"](h, now_ns, ids.ctypes.data, len(ids), spk_ptr, k, bwe_ptr, s, stream_ptr)
    if rc != 0:
        raise EngineError("room_summaries_enqueue rc=%d" % rc)


def downtrack_summaries(api, h):
    """lkf_downtrack_summaries: one DT_SUMMARY_DTYPE row per DownTrack handle."""
    n = C.c_uint32()
    rc = api["downtrack_summaries"](h, None, 0, C.byref(n))
    if rc not in (0, -28):
        raise EngineError("downtrack_summaries rc=%d" % rc)
    out = np.zeros(max(1, n.value), dtype=abi.DT_SUMMARY_DTYPE)
    rc = api["downtrack_summaries"](h, out.ctypes.data, n.value, C.byref(n))
    if rc != 0:
        raise EngineError("downtrack_summaries rc=%d" % rc)
    return out[:n.value]


def sender_stats(api, h, dts):
    """lkf_sender_stats_get for each DownTrack handle in `dts`: SENDER_STATS_DTYPE rows."""
    out = np.zeros(len(dts), dtype=abi.SENDER_STATS_DTYPE)
    for i, d in enumerate(dts):
        rc = api["sender_stats_get"](h, int(d), out[i:i + 1].ctypes.data)
        if rc != 0:
            raise EngineError("sender_stats_get(%d) rc=%d" % (d, rc))
    return out


def stream_stats(api, h, sid):
    st = abi.lkf_stream_stats()
    rc = api["stream_stats_get"](h, sid, C.byref(st))
    if rc != 0:
        raise EngineError("stream_stats_get rc=%d" % rc)
    return st.as_tuple()


class Engine:
    """One lkf_engine on one HIP device (one process per GPU)."""

    def __init__(self, device=0, max_tracks=1024, max_downtracks=16384, max_batch_pkts=1 << 16,
                 max_batch_arena=64 << 20, max_out_pkts=1 << 20, max_out_bytes=256 << 20,
                 max_batch_tuples=1 << 21, seq_size=500, lib_path=None):
        self.lib = load_library(lib_path)
        self.api = self.lib.api
        cfg = abi.lkf_cfg(max_tracks=max_tracks, max_downtracks=max_downtracks, max_batch_pkts=max_batch_pkts,
                          seq_size=seq_size, max_batch_arena=max_batch_arena, max_out_bytes=max_out_bytes,
                          max_out_pkts=max_out_pkts, max_batch_tuples=max_batch_tuples)
        self.h = self.lib.lkf_create(device, C.byref(cfg))
        if not self.h:
            raise EngineError("lkf_create failed on HIP device %d (no GPU or out of memory)" % device)
        self._srtcp_lens = np.zeros(0, dtype=np.uint32)  # the last srtcp_unprotect's plaintext lengths

    @classmethod
    def for_trace(cls, trace, device=0, headroom=1.25, extra_dts=0, **kw):
        """Engine sized for a synthetic `workload.Trace` (extra_dts: DownTracks
        added beyond the trace's, e.g. re-subscriptions)."""
        mp = int(trace.max_batch_pkts * headroom) + 64
        return cls(device=device, max_tracks=trace.ntracks + 8, max_downtracks=trace.ndts + 8 + extra_dts,
                   max_batch_pkts=mp, max_batch_arena=int(trace.max_batch_arena * headroom) + 4096,
                   max_batch_tuples=int(trace.max_batch_tuples * headroom) + 1024,
                   max_out_pkts=int(trace.max_batch_tuples * headroom) + 1024,
                   max_out_bytes=int(trace.max_batch_out_bytes * headroom) + (1 << 20), **kw)

    def _chk(self, rc, what):
        if rc != 0:
            raise EngineError("%s rc=%d: %s" % (what, rc, self.lib.lkf_last_error(self.h).decode()))

    def submit(self, pkts, n, arena, arena_len, dd=None):
        """lkf_submit (+ lkf_submit_dd with the batch's lkf_pkt_dd side array)."""
        self._chk(self.lib.lkf_submit(self.h, C.cast(pkts, C.c_void_p), n, C.cast(arena, C.c_void_p), arena_len),
                  "submit")
        if dd is not None:
            self._chk(self.api["submit_dd"](self.h, C.cast(dd, C.c_void_p), n), "submit_dd")

    def submit_device(self, d_pkts, n, d_arena, arena_len):
        self._chk(self.lib.lkf_submit_device(self.h, d_pkts, n, d_arena, arena_len), "submit_device")

    def run(self, stream=None):
        self._chk(self.lib.lkf_run(self.h, stream), "run")

    def ctl_key(self, dt, op, a0=0, a1=0, a2=0, a3=0, kind=abi.LKF_AT_ARRIVAL_NS, key=0):
        """lkf_ctl_key: a control op whose position in the next run's batch is
        a datagram index of the raw batch (abi.LKF_AT_DATAGRAM) or an arrival
        time (abi.LKF_AT_ARRIVAL_NS), resolved on the device."""
        self._chk(self.api["ctl_key"](self.h, dt, op, a0, a1, a2, a3, kind, key), "ctl_key")

    def ctl_batch_key(self, events):
        """lkf_ctl_batch_key: a ctypes array of abi.lkf_ctl_event_key, or a
        sequence of (dt, op, (a0, a1, a2, a3), kind, key)."""
        if not isinstance(events, C.Array):
            arr = (abi.lkf_ctl_event_key * max(1, len(events)))()
            for i, (dt, op, a, kind, key) in enumerate(events):
                arr[i].dt, arr[i].op, arr[i].kind, arr[i].key = dt, op, kind, key
                for j in range(4):
                    arr[i].a[j] = a[j]
            n = len(events)
            events = arr
        else:
            n = len(events)
        self._chk(self.api["ctl_batch_key"](self.h, C.cast(events, C.c_void_p), n), "ctl_batch_key")

    def ingest(self, raws, n, raw, raw_len):
        """Buffer.calc over a raw batch; the ExtPackets become the next run's batch."""
        rc = self.api["ingest"](self.h, C.cast(raws, C.c_void_p), n, C.cast(raw, C.c_void_p), raw_len)
        if rc != 0:
            raise EngineError("lkf_ingest rc=%d: %s" % (rc, self.lib.lkf_last_error(self.h).decode()))

    def ingest_device(self, d_raws, n, d_raw, raw_len):
        """lkf_ingest with HBM-resident raw datagrams (no host sync)."""
        rc = self.api["ingest_device"](self.h, d_raws, n, d_raw, raw_len)
        if rc != 0:
            raise EngineError("lkf_ingest_device rc=%d: %s" % (rc, self.lib.lkf_last_error(self.h).decode()))

    def set_stream_transport(self, stream, transport):
        """lkf_set_stream_transport: the transport (lkf_add_transport handle,
        -1: none) a received stream's datagrams are protected with."""
        self._chk(self.api["set_stream_transport"](self.h, stream, transport), "set_stream_transport")

    def unprotect_device(self, d_pkts, n, d_srtp, srtp_len, d_pkts_out, d_plain):
        """lkf_unprotect_device: SRTP unprotect of HBM-resident datagrams into
        (d_pkts_out, d_plain), the input of ingest_device (no host sync)."""
        self._chk(self.api["unprotect_device"](self.h, d_pkts, n, d_srtp, srtp_len, d_pkts_out, d_plain),
                  "unprotect_device")

    def ingest_srtp(self, raws, n, srtp, srtp_len):
        """lkf_ingest_srtp: the host form, unprotect then ingest."""
        self._chk(self.api["ingest_srtp"](self.h, C.cast(raws, C.c_void_p), n, C.cast(srtp, C.c_void_p), srtp_len),
                  "ingest_srtp")

    def unprotect_results(self):
        """lkf_unprotect_results -> abi.SRTP_RX_RESULT_DTYPE array, one row per datagram of the last unprotect."""
        n = C.c_uint32()
        rc = self.api["unprotect_results"](self.h, None, 0, C.byref(n))
        if rc not in (0, -28):
            self._chk(rc, "unprotect_results probe")
        out = np.zeros(n.value, dtype=abi.SRTP_RX_RESULT_DTYPE)
        self._chk(self.api["unprotect_results"](self.h, out.ctypes.data, n.value, C.byref(n)), "unprotect_results")
        return out

    def stream_srtp(self, stream):
        """lkf_stream_srtp_get -> (s_l, mask, started, transport, accepted, auth_failures, replays, malformed)."""
        st = abi.lkf_stream_srtp()
        self._chk(self.api["stream_srtp_get"](self.h, stream, C.byref(st)), "stream_srtp_get")
        return st.as_tuple()

    def unprotect_timing_window(self, n):
        ms = C.c_float()
        self._chk(self.api["unprotect_timing_window"](self.h, n, C.byref(ms)), "unprotect_timing_window")
        return ms.value

    def protect_timing_window(self, n):
        ms = C.c_float()
        self._chk(self.api["protect_timing_window"](self.h, n, C.byref(ms)), "protect_timing_window")
        return ms.value

    def flows(self):
        return flows_array(self.api, self.h)

    def stream_stats(self, sid):
        return stream_stats(self.api, self.h, sid)

    def speakers(self, now_ns):
        return speakers_array(self.api, self.h, now_ns)

    def sync(self):
        self._chk(self.lib.lkf_sync(self.h), "sync")

    def rtcp_feedback(self, entries, now_ns):
        """lkf_rtcp_feedback: `entries` an abi.RTCP_FB_DTYPE array grouped by
        DownTrack -> abi.RTCP_FB_RESULT_DTYPE array (one row per entry)."""
        ent = np.ascontiguousarray(entries, dtype=abi.RTCP_FB_DTYPE)
        out = np.zeros(len(ent), dtype=abi.RTCP_FB_RESULT_DTYPE)
        self._chk(self.api["rtcp_feedback"](self.h, ent.ctypes.data, len(ent), now_ns, out.ctypes.data),
                  "rtcp_feedback")
        return out

    def rtcp_ingest(self, raws, arena, now_ns):
        """lkf_rtcp_ingest: `raws` an abi.RTCP_RAW_DTYPE array grouped by
        DownTrack, `arena` the compound packets' bytes (bytes or a uint8
        array) -> (abi.RTCP_IN_RESULT_DTYPE per entry, abi.RTCP_FB_DTYPE
        records, their abi.RTCP_FB_RESULT_DTYPE results, abi.RTCP_REF_DTYPE
        records, the NACK list's length).  The lists are sized from the bytes
        (a report block is 24 bytes, a pass-through packet at least 20)."""
        rw = np.ascontiguousarray(raws, dtype=abi.RTCP_RAW_DTYPE)
        ar = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else \
            np.ascontiguousarray(arena, dtype=np.uint8)
        ln = rw["len"].astype(np.int64)
        fb_cap = int(np.maximum(1, ln // 24).sum())
        ref_cap = int((ln // 20).sum())
        out = np.zeros(len(rw), dtype=abi.RTCP_IN_RESULT_DTYPE)
        fb = np.zeros(max(1, fb_cap), dtype=abi.RTCP_FB_DTYPE)
        fbo = np.zeros(max(1, fb_cap), dtype=abi.RTCP_FB_RESULT_DTYPE)
        refs = np.zeros(max(1, ref_cap), dtype=abi.RTCP_REF_DTYPE)
        nfb, nref, nn = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.api["rtcp_ingest"](self.h, rw.ctypes.data, len(rw), ar.ctypes.data if len(ar) else None,
                                          len(ar), now_ns, out.ctypes.data, fb.ctypes.data, fbo.ctypes.data,
                                          len(fb), C.byref(nfb), refs.ctypes.data, len(refs), C.byref(nref),
                                          C.byref(nn)), "rtcp_ingest")
        return out, fb[:nfb.value], fbo[:nfb.value], refs[:nref.value], nn.value

    def srtcp_unprotect(self, raws, arena, want_plain=True):
        """lkf_srtcp_unprotect: `raws` an abi.SRTCP_RAW_DTYPE array, `arena`
        the datagrams' bytes (bytes or a uint8 array) ->
        (abi.SRTCP_RX_RESULT_DTYPE per datagram, the plaintext arena as a
        uint8 array of the input's length, or None)."""
        rw = np.ascontiguousarray(raws, dtype=abi.SRTCP_RAW_DTYPE)
        ar = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else \
            np.ascontiguousarray(arena, dtype=np.uint8)
        out = np.zeros(len(rw), dtype=abi.SRTCP_RX_RESULT_DTYPE)
        plain = np.zeros(len(ar), dtype=np.uint8) if want_plain else None
        self._chk(self.api["srtcp_unprotect"](self.h, rw.ctypes.data, len(rw), ar.ctypes.data if len(ar) else None,
                                              len(ar), plain.ctypes.data if want_plain and len(ar) else None,
                                              out.ctypes.data), "srtcp_unprotect")
        self._srtcp_lens = out["len"].copy()
        return out, plain

    def rtcp_ingest_unprotected(self, entries, now_ns):
        """lkf_rtcp_ingest_unprotected: `entries` an abi.RTCP_ENTRY_DTYPE array
        grouped by DownTrack, naming datagrams of the last srtcp_unprotect ->
        what rtcp_ingest returns.  The lists are sized from that call's
        plaintext lengths (`_srtcp_lens`)."""
        en = np.ascontiguousarray(entries, dtype=abi.RTCP_ENTRY_DTYPE)
        ln = np.zeros(len(en), dtype=np.int64)
        if len(en) and len(self._srtcp_lens):  # (a dgram out of range is the call's to refuse)
            ln = np.take(self._srtcp_lens, en["dgram"], mode="clip").astype(np.int64)
        fb_cap = int(np.maximum(1, ln // 24).sum())
        ref_cap = int((ln // 20).sum())
        out = np.zeros(len(en), dtype=abi.RTCP_IN_RESULT_DTYPE)
        fb = np.zeros(max(1, fb_cap), dtype=abi.RTCP_FB_DTYPE)
        fbo = np.zeros(max(1, fb_cap), dtype=abi.RTCP_FB_RESULT_DTYPE)
        refs = np.zeros(max(1, ref_cap), dtype=abi.RTCP_REF_DTYPE)
        nfb, nref, nn = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._chk(self.api["rtcp_ingest_unprotected"](self.h, en.ctypes.data, len(en), now_ns, out.ctypes.data,
                                                      fb.ctypes.data, fbo.ctypes.data, len(fb), C.byref(nfb),
                                                      refs.ctypes.data, len(refs), C.byref(nref), C.byref(nn)),
                  "rtcp_ingest_unprotected")
        return out, fb[:nfb.value], fbo[:nfb.value], refs[:nref.value], nn.value

    def set_downtrack_rtcp_transport(self, dt, transport):
        """lkf_set_downtrack_rtcp_transport: the transport DownTrack `dt`'s
        subscriber sends its RTCP on (-1: none)."""
        self._chk(self.api["set_downtrack_rtcp_transport"](self.h, dt, transport), "set_downtrack_rtcp_transport")

    def _rtcp_demux(self, what, n, call):
        # sized by the call itself: once for the count, again on LKF_ENOSPC (the calls keep no state)
        res = np.zeros(n, dtype=abi.RTCP_DMX_RESULT_DTYPE)
        ent = np.zeros(max(1, n), dtype=abi.RTCP_ENTRY_DTYPE)
        k = C.c_uint32()
        rc = call(res, ent, k)
        if rc == -28:  # LKF_ENOSPC
            ent = np.zeros(k.value, dtype=abi.RTCP_ENTRY_DTYPE)
            rc = call(res, ent, k)
        self._chk(rc, what)
        return res, ent[:k.value]

    def rtcp_demux(self, raws, arena):
        """lkf_rtcp_demux: `raws` an abi.SRTCP_RAW_DTYPE array {transport, off,
        len} of plaintext compounds in `arena` -> (abi.RTCP_DMX_RESULT_DTYPE
        per datagram, abi.RTCP_ENTRY_DTYPE entries sorted by DownTrack, then
        datagram)."""
        rw = np.ascontiguousarray(raws, dtype=abi.SRTCP_RAW_DTYPE)
        ar = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else \
            np.ascontiguousarray(arena, dtype=np.uint8)
        return self._rtcp_demux("rtcp_demux", len(rw), lambda res, ent, k: self.api["rtcp_demux"](
            self.h, rw.ctypes.data, len(rw), ar.ctypes.data if len(ar) else None, len(ar), res.ctypes.data,
            ent.ctypes.data, len(ent), C.byref(k)))

    def rtcp_demux_unprotected(self):
        """lkf_rtcp_demux_unprotected on the last srtcp_unprotect's plaintext
        -> what rtcp_demux returns; the entries pass to
        rtcp_ingest_unprotected unchanged."""
        return self._rtcp_demux("rtcp_demux_unprotected", len(self._srtcp_lens),
                                lambda res, ent, k: self.api["rtcp_demux_unprotected"](
                                    self.h, res.ctypes.data, ent.ctypes.data, len(ent), C.byref(k)))

    def transport_srtcp(self, transport):
        """lkf_transport_srtcp_get -> (slots [(in_use, ssrc, latest, mask)] * 16, the six counters)."""
        st = abi.lkf_transport_srtcp()
        self._chk(self.api["transport_srtcp_get"](self.h, transport, C.byref(st)), "transport_srtcp_get")
        return st.as_tuple()

    def srtcp_reset(self, transport):
        self._chk(self.api["srtcp_reset"](self.h, transport), "srtcp_reset")

    def srtcp_protect(self, raws, plain):
        """lkf_srtcp_protect: `raws` an abi.SRTCP_RAW_DTYPE array of plaintext
        compound packets in `plain` -> (abi.SRTCP_TX_RESULT_DTYPE per packet,
        the protected arena as a uint8 array of out_len bytes)."""
        rw = np.ascontiguousarray(raws, dtype=abi.SRTCP_RAW_DTYPE)
        ar = np.frombuffer(plain, dtype=np.uint8) if isinstance(plain, (bytes, bytearray)) else \
            np.ascontiguousarray(plain, dtype=np.uint8)
        cap = int(((rw["len"].astype(np.int64) + 35) & ~15).sum())
        out = np.zeros(max(1, cap), dtype=np.uint8)
        res = np.zeros(len(rw), dtype=abi.SRTCP_TX_RESULT_DTYPE)
        n = C.c_uint64()
        self._chk(self.api["srtcp_protect"](self.h, rw.ctypes.data, len(rw), ar.ctypes.data if len(ar) else None,
                                            len(ar), out.ctypes.data, cap, res.ctypes.data, C.byref(n)),
                  "srtcp_protect")
        return res, out[:n.value]

    def srtcp_tx_index(self, transport, ssrc):
        k = C.c_uint32()
        self._chk(self.api["srtcp_tx_index"](self.h, transport, ssrc, C.byref(k)), "srtcp_tx_index")
        return k.value

    def _ingested_nack_count(self):
        k = C.c_uint32()
        rc = self.api["rtcp_ingested_nacks"](self.h, None, 0, C.byref(k))
        if rc != -28:  # LKF_ENOSPC: the list is not empty
            self._chk(rc, "rtcp_ingested_nacks")
        return k.value

    def rtcp_ingested_nacks(self):
        """lkf_rtcp_ingested_nacks: the last rtcp_ingest's NACK list -> abi.NACK_DTYPE array."""
        k = C.c_uint32(self._ingested_nack_count())
        out = np.zeros(k.value, dtype=abi.NACK_DTYPE)
        if k.value:
            self._chk(self.api["rtcp_ingested_nacks"](self.h, out.ctypes.data, len(out), C.byref(k)),
                      "rtcp_ingested_nacks")
        return out

    def rtx_lookup_ingested(self, now_ns):
        """lkf_rtx_lookup_ingested: the RTX records of the device-resident NACK
        list -> abi.RTX_DTYPE array (one lookup: at most one record per NACK)."""
        k = C.c_uint32()
        out = np.zeros(max(1, self._ingested_nack_count()), dtype=abi.RTX_DTYPE)
        self._chk(self.api["rtx_lookup_ingested"](self.h, now_ns, out.ctypes.data, len(out), C.byref(k)),
                  "rtx_lookup_ingested")
        return out[:k.value]

    def rtcp_sender_reports(self, reqs, now_ns, wire=False):
        """lkf_rtcp_sender_reports: `reqs` an abi.RTCP_SR_REQ_DTYPE array ->
        abi.RTCP_SR_DTYPE array, and with wire=True also a uint8 [n, 28] array
        of the marshalled packets."""
        rq = np.ascontiguousarray(reqs, dtype=abi.RTCP_SR_REQ_DTYPE)
        out = np.zeros(len(rq), dtype=abi.RTCP_SR_DTYPE)
        w = np.zeros((len(rq), 28), dtype=np.uint8) if wire else None
        self._chk(self.api["rtcp_sender_reports"](self.h, rq.ctypes.data, len(rq), now_ns, out.ctypes.data,
                                                  w.ctypes.data if wire else None), "rtcp_sender_reports")
        return (out, w) if wire else out

    def sender_delta_info(self, dts):
        """lkf_sender_delta_info for the DownTrack handles `dts` -> abi.RTP_DELTA_INFO_DTYPE array."""
        d = np.ascontiguousarray(dts, dtype=np.int32)
        out = np.zeros(len(d), dtype=abi.RTP_DELTA_INFO_DTYPE)
        self._chk(self.api["sender_delta_info"](self.h, d.ctypes.data, len(d), out.ctypes.data), "sender_delta_info")
        return out

    def sender_rtcp(self, dts):
        """lkf_sender_rtcp_get for each DownTrack handle in `dts` -> abi.SENDER_RTCP_DTYPE array."""
        out = np.zeros(len(dts), dtype=abi.SENDER_RTCP_DTYPE)
        for i, d in enumerate(dts):
            self._chk(self.api["sender_rtcp_get"](self.h, int(d), out[i:i + 1].ctypes.data), "sender_rtcp_get")
        return out

    # ---- the publisher RTCP loop ----
    def stream_sender_reports(self, entries, now_ns):
        """lkf_stream_sender_reports: `entries` an abi.STREAM_SR_DTYPE array
        {stream, rtp, ntp} grouped by stream -> abi.STREAM_SR_RESULT_DTYPE
        array (one row per entry)."""
        ent = np.ascontiguousarray(entries, dtype=abi.STREAM_SR_DTYPE)
        out = np.zeros(len(ent), dtype=abi.STREAM_SR_RESULT_DTYPE)
        self._chk(self.api["stream_sender_reports"](self.h, ent.ctypes.data, len(ent), now_ns, out.ctypes.data),
                  "stream_sender_reports")
        return out

    def stream_receiver_reports(self, reqs, now_ns, wire=False):
        """lkf_stream_receiver_reports: `reqs` an abi.STREAM_RR_REQ_DTYPE array
        -> abi.STREAM_RR_DTYPE array, and with wire=True also a uint8 [n, 32]
        array of the marshalled rtcp.ReceiverReport packets."""
        rq = np.ascontiguousarray(reqs, dtype=abi.STREAM_RR_REQ_DTYPE)
        out = np.zeros(len(rq), dtype=abi.STREAM_RR_DTYPE)
        w = np.zeros((len(rq), 32), dtype=np.uint8) if wire else None
        self._chk(self.api["stream_receiver_reports"](self.h, rq.ctypes.data, len(rq), now_ns, out.ctypes.data,
                                                      w.ctypes.data if wire else None), "stream_receiver_reports")
        return (out, w) if wire else out

    def stream_rtcp_ingest(self, raws, arena, now_ns):
        """lkf_stream_rtcp_ingest: `raws` an abi.STREAM_RTCP_RAW_DTYPE array
        grouped by stream, `arena` the publishers' compound packets (bytes or a
        uint8 array) -> abi.STREAM_RTCP_IN_RESULT_DTYPE array."""
        rw = np.ascontiguousarray(raws, dtype=abi.STREAM_RTCP_RAW_DTYPE)
        ar = np.frombuffer(arena, dtype=np.uint8) if isinstance(arena, (bytes, bytearray)) else \
            np.ascontiguousarray(arena, dtype=np.uint8)
        out = np.zeros(len(rw), dtype=abi.STREAM_RTCP_IN_RESULT_DTYPE)
        self._chk(self.api["stream_rtcp_ingest"](self.h, rw.ctypes.data, len(rw), ar.ctypes.data if len(ar) else None,
                                                 len(ar), now_ns, out.ctypes.data), "stream_rtcp_ingest")
        return out

    def stream_rtcp_ingest_unprotected(self, entries, now_ns):
        """lkf_stream_rtcp_ingest_unprotected: `entries` an
        abi.STREAM_RTCP_ENTRY_DTYPE array grouped by stream, naming datagrams of
        the last srtcp_unprotect -> what stream_rtcp_ingest returns."""
        en = np.ascontiguousarray(entries, dtype=abi.STREAM_RTCP_ENTRY_DTYPE)
        out = np.zeros(len(en), dtype=abi.STREAM_RTCP_IN_RESULT_DTYPE)
        self._chk(self.api["stream_rtcp_ingest_unprotected"](self.h, en.ctypes.data, len(en), now_ns,
                                                             out.ctypes.data), "stream_rtcp_ingest_unprotected")
        return out

    def ingest_nacks_wire(self):
        """lkf_ingest_nacks_wire: the last ingest's NACKs as marshalled
        rtcp.TransportLayerNack packets -> (abi.STREAM_RTCP_PKT_DTYPE array,
        the packets' bytes as a uint8 array).  Sized by the call itself."""
        n, alen = C.c_uint32(), C.c_uint64()
        rc = self.api["ingest_nacks_wire"](self.h, None, 0, None, 0, C.byref(n), C.byref(alen))
        if rc != -28:  # LKF_ENOSPC: there are packets
            self._chk(rc, "ingest_nacks_wire")
        pk = np.zeros(n.value, dtype=abi.STREAM_RTCP_PKT_DTYPE)
        ar = np.zeros(alen.value, dtype=np.uint8)
        if n.value:
            self._chk(self.api["ingest_nacks_wire"](self.h, pk.ctypes.data, len(pk), ar.ctypes.data, len(ar),
                                                    C.byref(n), C.byref(alen)), "ingest_nacks_wire")
        return pk, ar

    def stream_fps_enable(self, stream):
        """lkf_stream_fps_enable: the VP8 / VP9 frame-rate calculators of a
        received stream, from the next ingest on."""
        self._chk(self.api["stream_fps_enable"](self.h, int(stream)), "stream_fps_enable")

    def stream_fps_get(self, stream):
        """lkf_stream_fps_get -> abi.lkf_stream_fps (fps[s][t] =
        GetTemporalLayerFpsForSpatial(s)[t]; as_dict() for exact compares)."""
        st = abi.lkf_stream_fps()
        self._chk(self.api["stream_fps_get"](self.h, int(stream), C.byref(st)), "stream_fps_get")
        return st

    def stream_fps_enable_dd(self, stream):
        """lkf_stream_fps_enable_dd: the dependency-descriptor frame-rate
        calculator of a received stream with dd_ext, from the next ingest on."""
        self._chk(self.api["stream_fps_enable_dd"](self.h, int(stream)), "stream_fps_enable_dd")

    def stream_fps_dd_get(self, stream):
        """lkf_stream_fps_dd_get -> abi.lkf_fps_dd (as_dict() for exact compares)."""
        st = abi.lkf_fps_dd()
        self._chk(self.api["stream_fps_dd_get"](self.h, int(stream), C.byref(st)), "stream_fps_dd_get")
        return st

    def ingest_fps_changed(self):
        """lkf_ingest_fps_changed: the streams that became calculated during
        the last ingest (OnFpsChanged), ascending, as a list of handles."""
        n = C.c_uint32()
        rc = self.api["ingest_fps_changed"](self.h, None, 0, C.byref(n))
        if rc != -28:  # LKF_ENOSPC: there are streams
            self._chk(rc, "ingest_fps_changed")
        out = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._chk(self.api["ingest_fps_changed"](self.h, out.ctypes.data, len(out), C.byref(n)),
                      "ingest_fps_changed")
        return [int(x) for x in out[:n.value]]

    def stream_rtcp(self, streams):
        """lkf_stream_rtcp_get for each stream handle in `streams` -> abi.STREAM_RTCP_DTYPE array."""
        out = np.zeros(len(streams), dtype=abi.STREAM_RTCP_DTYPE)
        for i, s in enumerate(streams):
            self._chk(self.api["stream_rtcp_get"](self.h, int(s), out[i:i + 1].ctypes.data), "stream_rtcp_get")
        return out

    def stats(self):
        st = abi.lkf_stats()
        self._chk(self.api["get_stats"](self.h, C.byref(st)), "get_stats")
        return st.as_dict()

    def drain(self):
        return drain_arrays(self.api, self.h)

    def drain_run_into(self, age, out_ptr, cap, arena_ptr, arena_cap):
        """lkf_drain_run into caller buffers (e.g. pinned host memory) -> (records, bytes)."""
        n = C.c_uint64()
        alen = C.c_uint64()
        f = self.lib.lkf_drain_run
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._chk(f(self.h, age, out_ptr, cap, arena_ptr, arena_cap, C.byref(n), C.byref(alen)), "drain_run")
        return n.value, alen.value

    def drain_run_async(self, age, out_ptr, cap, arena_ptr, arena_cap):
        """lkf_drain_run_async into page-locked buffers: returns (records, bytes)
        once the copies are enqueued; drain_wait() before reading them."""
        n = C.c_uint64()
        alen = C.c_uint64()
        f = self.lib.lkf_drain_run_async
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._chk(f(self.h, age, out_ptr, cap, arena_ptr, arena_cap, C.byref(n), C.byref(alen)), "drain_run_async")
        return n.value, alen.value

    def drain_wait(self):
        self.lib.lkf_drain_wait.restype = C.c_int
        self.lib.lkf_drain_wait.argtypes = [C.c_void_p]
        self._chk(self.lib.lkf_drain_wait(self.h), "drain_wait")

    def set_egress(self, mode):
        """lkf_set_egress: abi.LKF_EGRESS_WIRE (whole wire packets, the default)
        or abi.LKF_EGRESS_PREFIX (lkf_pre records + created bytes only) for the
        next runs."""
        self._chk(self.api["set_egress"](self.h, mode), "set_egress")

    def drain_prefix(self):
        """lkf_drain_prefix -> (records PRE_DTYPE, prefix arena) of the last run."""
        n = C.c_uint64()
        alen = C.c_uint64()
        rc = self.api["drain_prefix"](self.h, None, 0, None, 0, C.byref(n), C.byref(alen))
        if rc not in (0, -28):  # -28: ENOSPC for the size probe
            self._chk(rc, "drain_prefix probe")
        recs = np.zeros(n.value, dtype=abi.PRE_DTYPE)
        arena = np.zeros(alen.value, dtype=np.uint8)
        self._chk(self.api["drain_prefix"](self.h, recs.ctypes.data, n.value, arena.ctypes.data, alen.value,
                                           C.byref(n), C.byref(alen)), "drain_prefix")
        return recs, arena

    def drain_prefix_run_into(self, age, out_ptr, cap, arena_ptr, arena_cap):
        """lkf_drain_prefix_run into caller buffers (e.g. pinned host memory) -> (records, bytes)."""
        n = C.c_uint64()
        alen = C.c_uint64()
        self._chk(self.api["drain_prefix_run"](self.h, age, out_ptr, cap, arena_ptr, arena_cap, C.byref(n),
                                               C.byref(alen)), "drain_prefix_run")
        return n.value, alen.value

    def output_prefix_device(self):
        d_out = C.c_void_p()
        d_ar = C.c_void_p()
        n = C.c_uint64()
        alen = C.c_uint64()
        self._chk(self.api["output_prefix_device"](self.h, C.byref(d_out), C.byref(n), C.byref(d_ar), C.byref(alen)),
                  "output_prefix_device")
        return d_out.value, n.value, d_ar.value, alen.value

    def output_device(self):
        d_out = C.c_void_p()
        d_ar = C.c_void_p()
        n = C.c_uint64()
        alen = C.c_uint64()
        self._chk(self.lib.lkf_output_device(self.h, C.byref(d_out), C.byref(n), C.byref(d_ar), C.byref(alen)),
                  "output_device")
        return d_out.value, n.value, d_ar.value, alen.value

    def timings(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._chk(self.lib.lkf_last_timings(self.h, C.byref(a), C.byref(b), C.byref(c)), "timings")
        return a.value, b.value, c.value

    def timing_window(self, n):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        self._chk(self.lib.lkf_timing_window(self.h, n, C.byref(a), C.byref(b), C.byref(c)), "timing_window")
        return a.value, b.value, c.value

    def cumulative(self, reset=False):
        st = abi.lkf_stats()
        self._chk(self.lib.lkf_get_cumulative(self.h, C.byref(st), 1 if reset else 0), "cumulative")
        return st.as_dict()

    def close(self):
        if self.h:
            self.lib.lkf_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
