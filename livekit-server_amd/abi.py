"""ctypes mirror of include/lkfwd.h and csrc/synth.h (plain C structs).

The Python layer is host plumbing only: it loads ``liblkfwd.so`` (the HIP
engine) and ``liblkfsynth.so`` (the synthetic workload generator) and gives the
tests / bench a typed view of the C-ABI.  There is no compute here and no
fallback: a missing library raises.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.join(HERE, "lib")


class lkf_cfg(C.Structure):
    _fields_ = [
        ("max_tracks", C.c_uint32),
        ("max_downtracks", C.c_uint32),
        ("max_batch_pkts", C.c_uint32),
        ("seq_size", C.c_uint32),
        ("max_batch_arena", C.c_uint64),
        ("max_out_bytes", C.c_uint64),
        ("max_out_pkts", C.c_uint64),
        ("max_batch_tuples", C.c_uint64),
        ("max_streams", C.c_uint32),
        ("reserved_cfg", C.c_uint32),
    ]


class lkf_stream_params(C.Structure):
    _fields_ = [
        ("track", C.c_int32),
        ("layer", C.c_int32),
        ("ssrc", C.c_uint32),
        ("audio_level_ext", C.c_uint8),
        ("active_level", C.c_uint8),
        ("min_percentile", C.c_uint8),
        ("dd_ext", C.c_uint8),
        ("observe_duration_ms", C.c_uint32),
        ("smooth_intervals", C.c_uint32),
        ("nack", C.c_uint8),
        ("twcc_ext", C.c_uint8),
        ("reserved", C.c_uint8 * 2),
        ("rtt_ms", C.c_uint32),
    ]


class lkf_raw_pkt(C.Structure):
    _fields_ = [
        ("arrival_ns", C.c_int64),
        ("stream", C.c_uint32),
        ("off", C.c_uint32),
        ("len", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class lkf_flow(C.Structure):
    _fields_ = [
        ("ext_sn", C.c_uint64),
        ("ext_ts", C.c_uint64),
        ("loss_start", C.c_uint64),
        ("loss_end", C.c_uint64),
        ("pkt", C.c_uint32),
        ("flags", C.c_uint8),
        ("reserved", C.c_uint8 * 3),
    ]


class lkf_stream_stats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "ext_start_sn", "ext_highest_sn", "ext_start_ts", "ext_highest_ts", "packets_lost",
        "packets_out_of_order", "packets_duplicate", "packets_padding", "bytes", "header_bytes",
        "bytes_duplicate", "bytes_padding", "frames", "nacks")] + [
            ("initialized", C.c_uint8), ("reserved", C.c_uint8 * 7),
            ("first_time_ns", C.c_int64), ("highest_time_ns", C.c_int64),
            ("last_transit", C.c_uint64), ("last_jitter_ext_ts", C.c_uint64),
            ("jitter", C.c_double), ("max_jitter", C.c_double),
            ("gap_histogram", C.c_uint32 * 101), ("reserved2", C.c_uint32)]

    def as_tuple(self):
        """Every field but the reserved ones (jitter as float64 bits: compared exactly)."""
        import struct
        out = []
        for n, _ in self._fields_:
            if n.startswith("reserved"):
                continue
            v = getattr(self, n)
            if n in ("jitter", "max_jitter"):
                v = struct.unpack("<Q", struct.pack("<d", v))[0]
            elif n == "gap_histogram":
                v = tuple(v)
            out.append(v)
        return tuple(out)


class lkf_speaker(C.Structure):
    _fields_ = [
        ("room", C.c_uint32),
        ("participant", C.c_uint32),
        ("level", C.c_float),
        ("active", C.c_uint32),
    ]


RTCP_NACK_DTYPE = np.dtype([("datagram", "<u4"), ("stream", "<u4"), ("media_ssrc", "<u4"), ("pair_off", "<u4"),
                            ("n_pairs", "<u2"), ("num_nacked", "<u2"), ("reserved", "<u4")])
assert RTCP_NACK_DTYPE.itemsize == 24
NACK_PAIR_DTYPE = np.dtype([("packet_id", "<u2"), ("lost_packets", "<u2")])
FLOW_DTYPE = np.dtype([("ext_sn", "<u8"), ("ext_ts", "<u8"), ("loss_start", "<u8"), ("loss_end", "<u8"),
                       ("pkt", "<u4"), ("flags", "u1"), ("reserved", "V3")])
assert FLOW_DTYPE.itemsize == 40
SPEAKER_DTYPE = np.dtype([("room", "<u4"), ("participant", "<u4"), ("level", "<f4"), ("active", "<u4")])
# lkf_dt_summary (per-DownTrack sendingPacket totals + lastAllocation.IsDeficient)
DT_SUMMARY_DTYPE = np.dtype([("dt", "<i4"), ("subscriber", "<u4"), ("room", "<u4"), ("flags", "<u4"),
                             ("packets_sent", "<u8"), ("bytes_sent", "<u8")])
assert DT_SUMMARY_DTYPE.itemsize == 32
# the cooperative allocation pass (lkf_prov_req / lkf_prov_result / lkf_alloc_group)
PROV_REQ_DTYPE = np.dtype([("dt", "<i4"), ("spatial", "<i4"), ("temporal", "<i4"), ("allow_pause", "u1"),
                           ("allow_overshoot", "u1"), ("reserved", "u1", 2), ("capacity", "<i8")])
assert PROV_REQ_DTYPE.itemsize == 24
PROV_RESULT_DTYPE = np.dtype([("dt", "<i4"), ("is_candidate", "u1"), ("reserved", "u1", 3), ("used", "<i8")])
assert PROV_RESULT_DTYPE.itemsize == 16
ALLOC_GROUP_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("capacity", "<i8"), ("allow_pause", "u1"),
                              ("allow_overshoot", "u1"), ("reserved", "u1", 6)])
assert ALLOC_GROUP_DTYPE.itemsize == 24
# lkf_dd_tracker_status (StreamTrackerDependencyDescriptor)
DD_TRACKER_STATUS_DTYPE = np.dtype([("tracker", "<i4"), ("max_spatial", "<i4"), ("max_temporal", "<i4"),
                                    ("bitrate_changed", "<u4"), ("notifications", "<u4", (3,)),
                                    ("last_notified", "<i4", (3,)), ("status", "u1", (3,)), ("worker", "u1"),
                                    ("reserved", "<u4"), ("bitrate", "<i8", (3, 4))])
assert DD_TRACKER_STATUS_DTYPE.itemsize == 144
# lkf_sender_stats (DownTrack.rtpStats = buffer.RTPStatsSender)
SENDER_STATS_DTYPE = np.dtype(
    [(f, "<u8") for f in ("ext_start_sn", "ext_highest_sn", "ext_start_ts", "ext_highest_ts")]
    + [("first_time_ns", "<i8"), ("highest_time_ns", "<i8"), ("last_transit", "<u8"), ("last_jitter_ext_ts", "<u8")]
    + [(f, "<u8") for f in ("bytes", "header_bytes", "bytes_duplicate", "header_bytes_duplicate", "bytes_padding",
                            "header_bytes_padding", "packets_duplicate", "packets_padding", "packets_out_of_order",
                            "packets_lost")]
    + [("jitter", "<f8"), ("max_jitter", "<f8")]
    + [(f, "<u4") for f in ("frames", "key_frames", "initialized", "clock_rate")]
    + [("gap_histogram", "<u4", (101,)), ("reserved", "<u4")])
assert SENDER_STATS_DTYPE.itemsize == 584


# ---- the DownTrack RTCP loop (lkf_rtcp_feedback / lkf_rtcp_sender_reports / lkf_sender_delta_info) ----
class lkf_rtcp_sr_data(C.Structure):
    _fields_ = [("ntp", C.c_uint64), ("rtp_ext", C.c_uint64), ("at_ns", C.c_int64), ("valid", C.c_uint32),
                ("reserved", C.c_uint32)]


class lkf_interval_stats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("packets", "bytes", "header_bytes", "packets_padding", "bytes_padding",
                                          "header_bytes_padding", "packets_lost", "packets_out_of_order",
                                          "packets_not_found")] + [("frames", C.c_uint32), ("reserved", C.c_uint32)]


class lkf_sender_snapshot(C.Structure):
    _fields_ = ([("is_valid", C.c_uint32), ("frames", C.c_uint32), ("start_time_ns", C.c_int64)]
                + [(f, C.c_uint64) for f in ("ext_start_sn", "bytes", "header_bytes", "packets_padding",
                                             "bytes_padding", "header_bytes_padding", "packets_duplicate",
                                             "bytes_duplicate", "header_bytes_duplicate", "packets_out_of_order",
                                             "packets_lost_feed", "packets_lost")]
                + [(f, C.c_uint32) for f in ("nacks", "plis", "firs", "max_rtt")]
                + [("max_jitter_feed", C.c_double), ("max_jitter", C.c_double), ("ext_last_rr_sn", C.c_uint64),
                   ("interval_stats", lkf_interval_stats)])


class lkf_sender_rtcp(C.Structure):
    _fields_ = ([("ext_highest_sn_from_rr", C.c_uint64), ("last_rr_time_ns", C.c_int64),
                 ("packets_lost_from_rr", C.c_uint64), ("jitter_from_rr", C.c_double),
                 ("max_jitter_from_rr", C.c_double), ("end_time_ns", C.c_int64)]
                + [(f, C.c_uint32) for f in ("last_rr_last_sequence_number", "last_rr_total_lost", "rtt", "max_rtt",
                                             "nacks", "plis", "firs", "clock_skew_count",
                                             "out_of_order_sender_report_count", "metadata_cache_overflow_count")]
                + [("sr_first", lkf_rtcp_sr_data), ("sr_newest", lkf_rtcp_sr_data),
                   ("snapshot", lkf_sender_snapshot)])


class lkf_rtcp_fb(C.Structure):
    _fields_ = ([("dt", C.c_int32)]
                + [(f, C.c_uint32) for f in ("flags", "last_sequence_number", "total_lost", "jitter",
                                             "last_sender_report", "delay", "nacks", "plis", "firs")]
                + [("fraction_lost", C.c_uint8), ("reserved", C.c_uint8 * 7)])


class lkf_rtcp_fb_result(C.Structure):
    _fields_ = [("rtt_ms", C.c_uint32), ("flags", C.c_uint32)]


class lkf_rtcp_sr_req(C.Structure):
    _fields_ = [("dt", C.c_int32), ("calculated_clock_rate", C.c_uint32)]


# RTCP ingress (lkf_rtcp_ingest)
class lkf_rtcp_raw(C.Structure):
    _fields_ = [("dt", C.c_int32), ("off", C.c_uint32), ("len", C.c_uint32)]


class lkf_rtcp_in_result(C.Structure):
    _fields_ = ([(f, C.c_uint32) for f in ("status", "rtt_ms", "fb_first", "fb_count", "reports", "nacks", "plis",
                                           "firs", "nack_first")]
                + [("pli_layer", C.c_int32), ("ref_first", C.c_uint32), ("ref_count", C.c_uint32)])


class lkf_rtcp_ref(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("entry", "kind", "off", "len")]


class lkf_rtcp_sr(C.Structure):
    _fields_ = [("dt", C.c_int32), ("flags", C.c_uint32), ("ntp", C.c_uint64), ("rtp_ext", C.c_uint64),
                ("rtp", C.c_uint32), ("packet_count", C.c_uint32), ("octet_count", C.c_uint32),
                ("reserved", C.c_uint32)]


class lkf_rtp_delta_info(C.Structure):
    _fields_ = ([("start_time_ns", C.c_int64), ("duration_ns", C.c_int64)]
                + [(f, C.c_uint64) for f in ("bytes", "header_bytes", "bytes_duplicate", "header_bytes_duplicate",
                                             "bytes_padding", "header_bytes_padding")]
                + [("jitter_max", C.c_double)]
                + [(f, C.c_uint32) for f in ("valid", "packets", "packets_duplicate", "packets_padding",
                                             "packets_lost", "packets_missing", "packets_out_of_order", "frames",
                                             "rtt_max", "nacks", "plis", "firs")])


def _dtype_of(struct):
    """The numpy dtype of a ctypes structure of integers, doubles, byte arrays and nested structures."""
    kinds = {C.c_uint64: "<u8", C.c_int64: "<i8", C.c_uint32: "<u4", C.c_int32: "<i4", C.c_double: "<f8",
             C.c_uint8: "u1"}
    out = []
    for name, t in struct._fields_:
        if t in kinds:
            out.append((name, kinds[t]))
        elif issubclass(t, C.Structure):
            out.append((name, _dtype_of(t)))
        else:  # a byte array
            out.append((name, "u1", (C.sizeof(t),)))
    return np.dtype(out)


LKF_FB_HAS_RR = 0x1
LKF_FB_RTT_CHANGED, LKF_FB_IGNORED, LKF_FB_CACHE_OVERFLOW = 0x1, 0x2, 0x4
LKF_SR_VALID, LKF_SR_CLOCK_SKEW, LKF_SR_REPAIRED = 0x1, 0x2, 0x4
SENDER_RTCP_DTYPE = _dtype_of(lkf_sender_rtcp)
RTCP_FB_DTYPE = _dtype_of(lkf_rtcp_fb)
RTCP_FB_RESULT_DTYPE = _dtype_of(lkf_rtcp_fb_result)
RTCP_SR_REQ_DTYPE = _dtype_of(lkf_rtcp_sr_req)
RTCP_SR_DTYPE = _dtype_of(lkf_rtcp_sr)
RTP_DELTA_INFO_DTYPE = _dtype_of(lkf_rtp_delta_info)
LKF_RTCP_IN_OK, LKF_RTCP_IN_MALFORMED = 0, 1
LKF_RTCP_MAX_LEN = 65535
LKF_RTCP_REF_REMB, LKF_RTCP_REF_TWCC = 1, 2
RTCP_RAW_DTYPE = _dtype_of(lkf_rtcp_raw)
RTCP_IN_RESULT_DTYPE = _dtype_of(lkf_rtcp_in_result)
RTCP_REF_DTYPE = _dtype_of(lkf_rtcp_ref)
assert C.sizeof(lkf_rtcp_raw) == 12 == RTCP_RAW_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_in_result) == 48 == RTCP_IN_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_ref) == 16 == RTCP_REF_DTYPE.itemsize
assert C.sizeof(lkf_sender_rtcp) == 384 == SENDER_RTCP_DTYPE.itemsize, C.sizeof(lkf_sender_rtcp)
assert C.sizeof(lkf_rtcp_fb) == 48 == RTCP_FB_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_fb_result) == 8 == RTCP_FB_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_sr_req) == 8 == RTCP_SR_REQ_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_sr) == 40 == RTCP_SR_DTYPE.itemsize
assert C.sizeof(lkf_rtp_delta_info) == 120 == RTP_DELTA_INFO_DTYPE.itemsize


# ---- the publisher RTCP loop (lkf_stream_sender_reports / lkf_stream_receiver_reports / lkf_stream_rtcp_ingest) ----
class lkf_stream_sr(C.Structure):
    _fields_ = [("stream", C.c_int32), ("rtp", C.c_uint32), ("ntp", C.c_uint64)]


class lkf_stream_sr_result(C.Structure):
    _fields_ = [("ntp", C.c_uint64), ("rtp_ext", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class lkf_stream_rr_req(C.Structure):
    _fields_ = [("stream", C.c_int32), ("proxy_fraction_lost", C.c_uint32)]


class lkf_stream_rr(C.Structure):
    _fields_ = [("stream", C.c_int32)] + [(f, C.c_uint32) for f in (
        "flags", "ssrc", "fraction_lost", "total_lost", "last_sequence_number", "jitter", "last_sender_report", "delay",
        "reserved")]


class lkf_stream_rtcp_raw(C.Structure):
    _fields_ = [("stream", C.c_int32), ("off", C.c_uint32), ("len", C.c_uint32)]


class lkf_stream_rtcp_entry(C.Structure):
    _fields_ = [("stream", C.c_int32), ("dgram", C.c_uint32)]


class lkf_stream_rtcp_in_result(C.Structure):
    _fields_ = ([(f, C.c_uint32) for f in ("status", "n_sr", "flags", "reserved")]
                + [("ntp", C.c_uint64), ("rtp_ext", C.c_uint64)])


class lkf_stream_rtcp_pkt(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("datagram", "stream", "off", "len")]


class lkf_stream_rtcp(C.Structure):
    _fields_ = [("sr_first", lkf_rtcp_sr_data), ("sr_newest", lkf_rtcp_sr_data), ("snapshot_is_valid", C.c_uint32),
                ("started", C.c_uint32), ("snapshot_start_time_ns", C.c_int64), ("snapshot_ext_start_sn", C.c_uint64),
                ("snapshot_packets_lost", C.c_uint64), ("start_time_ns", C.c_int64), ("clock_skew_count", C.c_uint32),
                ("out_of_order_sender_report_count", C.c_uint32)]


LKF_FPS_NONE, LKF_FPS_VP8, LKF_FPS_VP9, LKF_FPS_DD = 0, 1, 2, 3


class lkf_fps_calc(C.Structure):
    _fields_ = [("present", C.c_uint64), ("first", C.c_int8 * 4), ("second", C.c_int8 * 4), ("base_fn", C.c_uint16),
                ("has_base", C.c_uint8), ("reserved", C.c_uint8), ("resets", C.c_uint32)]


class lkf_stream_fps(C.Structure):
    _fields_ = [("fps", (C.c_float * 4) * 3), ("kind", C.c_uint32), ("calculated", C.c_uint8),
                ("completed", C.c_uint8 * 3), ("calc", lkf_fps_calc * 3)]

    def as_dict(self):
        """Every field, the rates as binary32 bits (compared exactly)."""
        import struct
        return {
            "kind": self.kind, "calculated": self.calculated, "completed": tuple(self.completed),
            "fps_bits": tuple(tuple(struct.unpack("<I", struct.pack("<f", v))[0] for v in row) for row in self.fps),
            "calc": tuple((c.present, tuple(c.first), tuple(c.second), c.base_fn, c.has_base, c.resets)
                          for c in self.calc)}


assert C.sizeof(lkf_fps_calc) == 24 and C.sizeof(lkf_stream_fps) == 128


class lkf_fps_dd(C.Structure):
    """FrameRateCalculatorDD's state (lkf_stream_fps_dd_get)."""
    _fields_ = [("base_fn", C.c_uint16), ("has_base", C.c_uint8), ("completed", C.c_uint8),
                ("max_spatial", C.c_uint8), ("max_temporal", C.c_uint8), ("reserved", C.c_uint16),
                ("resets", C.c_uint32), ("reserved2", C.c_uint32), ("present", C.c_uint64 * 4),
                ("first", (C.c_int16 * 4) * 3), ("second", (C.c_int16 * 4) * 3),
                ("chain", ((C.c_uint64 * 4) * 4) * 3)]

    def as_dict(self):
        return {
            "base_fn": self.base_fn, "has_base": self.has_base, "completed": self.completed,
            "max_spatial": self.max_spatial, "max_temporal": self.max_temporal, "resets": self.resets,
            "present": tuple(self.present), "first": tuple(tuple(r) for r in self.first),
            "second": tuple(tuple(r) for r in self.second),
            "chain": tuple(tuple(tuple(w) for w in row) for row in self.chain)}


assert C.sizeof(lkf_fps_dd) == 480

(LKF_SSR_IGNORED_UNINIT, LKF_SSR_ANACHRONOUS, LKF_SSR_CLOCK_SKEW, LKF_SSR_RESET_FIRST, LKF_SSR_FIRST_TIME_ADJUSTED,
 LKF_SSR_ADJUST_TOO_BIG, LKF_SSR_CLOSED) = (1 << k for k in range(7))
LKF_SRR_VALID = 0x1
STREAM_SR_DTYPE = _dtype_of(lkf_stream_sr)
STREAM_SR_RESULT_DTYPE = _dtype_of(lkf_stream_sr_result)
STREAM_RR_REQ_DTYPE = _dtype_of(lkf_stream_rr_req)
STREAM_RR_DTYPE = _dtype_of(lkf_stream_rr)
STREAM_RTCP_RAW_DTYPE = _dtype_of(lkf_stream_rtcp_raw)
STREAM_RTCP_ENTRY_DTYPE = _dtype_of(lkf_stream_rtcp_entry)
STREAM_RTCP_IN_RESULT_DTYPE = _dtype_of(lkf_stream_rtcp_in_result)
STREAM_RTCP_PKT_DTYPE = _dtype_of(lkf_stream_rtcp_pkt)
STREAM_RTCP_DTYPE = _dtype_of(lkf_stream_rtcp)
assert C.sizeof(lkf_stream_sr) == 16 == STREAM_SR_DTYPE.itemsize
assert C.sizeof(lkf_stream_sr_result) == 24 == STREAM_SR_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_stream_rr_req) == 8 == STREAM_RR_REQ_DTYPE.itemsize
assert C.sizeof(lkf_stream_rr) == 40 == STREAM_RR_DTYPE.itemsize
assert C.sizeof(lkf_stream_rtcp_raw) == 12 == STREAM_RTCP_RAW_DTYPE.itemsize
assert C.sizeof(lkf_stream_rtcp_entry) == 8 == STREAM_RTCP_ENTRY_DTYPE.itemsize
assert C.sizeof(lkf_stream_rtcp_in_result) == 32 == STREAM_RTCP_IN_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_stream_rtcp_pkt) == 16 == STREAM_RTCP_PKT_DTYPE.itemsize
assert C.sizeof(lkf_stream_rtcp) == 112 == STREAM_RTCP_DTYPE.itemsize
# NACK -> RTX (lkf_nack / lkf_rtx)
NACK_DTYPE = np.dtype([("dt", "<i4"), ("sn", "<u2"), ("reserved", "<u2")])
assert NACK_DTYPE.itemsize == 8
RTX_DTYPE = np.dtype([("ext_sn", "<u8"), ("ext_ts", "<u8"), ("source_sn", "<u2"), ("target_sn", "<u2"),
                      ("timestamp", "<u4"), ("last_nack", "<u4"), ("marker", "u1"), ("nacked", "u1"), ("layer", "i1"),
                      ("codec_len", "u1"), ("codec", "u1", 8), ("dt", "<i4"), ("reserved", "<u4")])
assert RTX_DTYPE.itemsize == 48
DTS_ACTIVE = 0x1
DTS_DEFICIENT = 0x2
# padding / blank frames (lkf_pad_req)
PAD_REQ_DTYPE = np.dtype([("dt", "<i4"), ("bytes_to_send", "<u4"), ("flags", "<u4"), ("start_sn", "<u4"),
                          ("start_ts", "<u4"), ("reserved", "<u4")])
assert PAD_REQ_DTYPE.itemsize == 24
ALLOC_REQ_DTYPE = np.dtype([("dt", "<i4"), ("available_layers", "<u4"), ("bitrates", "<i8", (3, 4)),
                            ("allow_overshoot", "u1"), ("reserved", "u1", 7)])
assert ALLOC_REQ_DTYPE.itemsize == 112
ALLOCATION_DTYPE = np.dtype([("dt", "<i4"), ("pause_reason", "<i4"), ("bandwidth_requested", "<i8"),
                             ("bandwidth_delta", "<i8"), ("bandwidth_needed", "<i8"), ("target_spatial", "<i4"),
                             ("target_temporal", "<i4"), ("request_spatial", "<i4"), ("max_spatial", "<i4"),
                             ("max_temporal", "<i4"), ("is_deficient", "u1"), ("boosted", "u1"),
                             ("reserved", "u1", 2),
                             ("distance_to_desired", "<f8")])
assert ALLOCATION_DTYPE.itemsize == 64
VIDEO_TRANSITION_DTYPE = np.dtype([("dt", "<i4"), ("from_spatial", "<i4"), ("from_temporal", "<i4"),
                                   ("to_spatial", "<i4"), ("to_temporal", "<i4"), ("available", "u1"),
                                   ("reserved", "u1", 3), ("bandwidth_delta", "<i8")])
assert VIDEO_TRANSITION_DTYPE.itemsize == 32
TRACKER_STATUS_DTYPE = np.dtype([("tracker", "<i4"), ("status", "u1"), ("bitrate_changed", "u1"), ("reserved", "u1", 2),
                                 ("notifications", "<u4"), ("reserved2", "<u4"), ("bitrate", "<i8", 4),
                                 ("cumulative", "<i8", 4)])
assert TRACKER_STATUS_DTYPE.itemsize == 80
TRACKER_RESET, TRACKER_PAUSE, TRACKER_STOP = 1, 2, 3
PAD_ON_MUTE = 0x1
PAD_FORCE_MARKER = 0x2
PAD_WRITABLE = 0x4
PAD_RR_SEEN = 0x8


class lkf_track_params(C.Structure):
    _fields_ = [
        ("track_id", C.c_uint64),
        ("room", C.c_uint32),
        ("publisher", C.c_uint32),
        ("kind", C.c_uint8),
        ("codec", C.c_uint8),
        ("has_ref_ts", C.c_uint8),
        ("is_mic", C.c_uint8),
        ("clock_rate", C.c_uint32),
        ("layer_offsets", (C.c_uint32 * 3) * 3),
        ("has_dd", C.c_uint8),
        ("reserved_tp", C.c_uint8 * 3),
    ]


class lkf_downtrack_params(C.Structure):
    _fields_ = [
        ("track", C.c_int32),
        ("subscriber", C.c_uint32),
        ("ssrc", C.c_uint32),
        ("payload_type", C.c_uint8),
        ("ext_dd", C.c_uint8),
        ("ext_playout", C.c_uint8),
        ("ext_abs_send_time", C.c_uint8),
        ("playout_delay", C.c_uint8 * 3),
        ("has_expected_ts", C.c_uint8),
        ("ext_transport_cc", C.c_uint8),
        ("reserved_dp", C.c_uint8 * 3),
        ("bind_time_ns", C.c_int64),
    ]


class lkf_pkt(C.Structure):
    _fields_ = [
        ("ext_sn", C.c_uint64),
        ("ext_ts", C.c_uint64),
        ("arrival_ns", C.c_int64),
        ("arena_off", C.c_uint32),
        ("track", C.c_uint32),
        ("ssrc", C.c_uint32),
        ("payload_off", C.c_uint16),
        ("payload_len", C.c_uint16),
        ("hdr0", C.c_uint8),
        ("hdr1", C.c_uint8),
        ("spatial", C.c_int8),
        ("temporal", C.c_int8),
        ("flags", C.c_uint8),
        ("vp8_first", C.c_uint8),
        ("vp8_bits", C.c_uint8),
        ("vp8_hdr_size", C.c_uint8),
        ("vp8_picture_id", C.c_uint16),
        ("vp8_tl0picidx", C.c_uint8),
        ("vp8_tid", C.c_uint8),
        ("vp8_keyidx", C.c_uint8),
        ("layer", C.c_int8),
        ("audio_level", C.c_uint8),
        ("vp9_bits", C.c_uint8),
        ("reserved", C.c_uint8 * 8),
    ]


class lkf_pkt_dd(C.Structure):
    _fields_ = [
        ("ext_frame_num", C.c_uint64),
        ("ext_key_frame_num", C.c_uint64),
        ("dd_off", C.c_uint16),
        ("dd_len", C.c_uint8),
        ("flags", C.c_uint8),
        ("reserved", C.c_uint32 * 3),
    ]


class lkf_out(C.Structure):
    _fields_ = [
        ("ext_sn", C.c_uint64),
        ("ext_ts", C.c_uint64),
        ("out_off", C.c_uint64),
        ("dt", C.c_uint32),
        ("pkt", C.c_uint32),
        ("out_len", C.c_uint16),
        ("flags", C.c_uint8),
        ("layer", C.c_int8),
        ("reserved", C.c_uint32),
    ]


class lkf_pre(C.Structure):  # prefix egress record (lkf_set_egress(LKF_EGRESS_PREFIX))
    _fields_ = [
        ("ext_sn", C.c_uint64),
        ("ext_ts", C.c_uint64),
        ("pre_off", C.c_uint64),
        ("dt", C.c_uint32),
        ("pkt", C.c_uint32),
        ("out_len", C.c_uint16),
        ("flags", C.c_uint8),
        ("layer", C.c_int8),
        ("pre_len", C.c_uint16),
        ("tail_len", C.c_uint16),
        ("tail_src", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


LKF_EGRESS_WIRE, LKF_EGRESS_PREFIX = 0, 1
LKF_DROP_NREASONS = 11
LKF_KIND_AUDIO, LKF_KIND_VIDEO = 0, 1  # enum lkf_kind
LKF_CTL_MUTE, LKF_CTL_PUBMUTE, LKF_CTL_SET_MAX_SPATIAL, LKF_CTL_SET_MAX_TEMPORAL = 1, 2, 3, 4
LKF_CTL_SET_MAX_SEEN_SPATIAL, LKF_CTL_SET_MAX_SEEN_TEMPORAL, LKF_CTL_SET_ALLOCATION = 5, 6, 7
LKF_CTL_RESYNC, LKF_CTL_SET_TARGET, LKF_CTL_PLAYOUT_ACKED = 8, 9, 10


class lkf_stats(C.Structure):
    _fields_ = [
        ("tuples", C.c_uint64),
        ("forwarded", C.c_uint64),
        ("out_bytes", C.c_uint64),
        ("arena_bytes", C.c_uint64),
        ("drops", C.c_uint64 * LKF_DROP_NREASONS),
    ]

    def as_dict(self):
        return {
            "tuples": self.tuples,
            "forwarded": self.forwarded,
            "out_bytes": self.out_bytes,
            "arena_bytes": self.arena_bytes,
            "drops": list(self.drops),
        }


class lkf_fwd_state(C.Structure):
    _fields_ = [
        ("started", C.c_uint8),
        ("last_marker", C.c_uint8),
        ("second_last_marker", C.c_uint8),
        ("has_vp8", C.c_uint8),
        ("reference_layer_spatial", C.c_int32),
        ("pre_start_time_ns", C.c_int64),
        ("ext_first_ts", C.c_uint64),
        ("ref_ts_offset", C.c_uint64),
        ("ext_last_sn", C.c_uint64),
        ("ext_second_last_sn", C.c_uint64),
        ("ext_last_ts", C.c_uint64),
        ("ext_second_last_ts", C.c_uint64),
        ("vp8_ext_last_picture_id", C.c_int32),
        ("vp8_picture_id_used", C.c_uint8),
        ("vp8_last_tl0picidx", C.c_uint8),
        ("vp8_tl0picidx_used", C.c_uint8),
        ("vp8_tid_used", C.c_uint8),
        ("vp8_last_keyidx", C.c_uint8),
        ("vp8_keyidx_used", C.c_uint8),
        ("pad", C.c_uint8 * 2),
    ]

    def as_tuple(self):
        return tuple(getattr(self, f[0]) for f in self._fields_ if f[0] != "pad")


class lkf_transport_params(C.Structure):
    _fields_ = [
        ("master_key", C.c_uint8 * 16),
        ("master_salt", C.c_uint8 * 14),
        ("profile", C.c_uint16),
    ]


LKF_SRTP_AES128_CM_HMAC_SHA1_80 = 1
LKF_SRTP_AEAD_AES_128_GCM = 2
LKF_TWCC_PUSH = 0x80000000
# lkf_flow.flags (LKF_FLOW_*)
LKF_FLOW_NOT_HANDLED, LKF_FLOW_DUPLICATE, LKF_FLOW_OUT_OF_ORDER, LKF_FLOW_HAS_LOSS = 0x01, 0x02, 0x04, 0x08
LKF_FLOW_PADDING, LKF_FLOW_FORWARD, LKF_FLOW_BAD, LKF_FLOW_BUCKET = 0x10, 0x20, 0x40, 0x80
LKF_TWCC_MARKER = 0x00010000
SRTP_TAG_LEN = 10
# SRTP unprotect (lkf_unprotect_device / lkf_ingest_srtp): per-datagram status, results and per-stream state
LKF_SRTP_RX_OK, LKF_SRTP_RX_MALFORMED, LKF_SRTP_RX_REPLAY_OLD, LKF_SRTP_RX_REPLAY_DUP, LKF_SRTP_RX_AUTH = 0, 1, 2, 3, 4
SRTP_RX_RESULT_DTYPE = np.dtype([("index", "<u8"), ("status", "<u4"), ("len", "<u4")])
assert SRTP_RX_RESULT_DTYPE.itemsize == 16
RAW_PKT_DTYPE = np.dtype([("arrival_ns", "<i8"), ("stream", "<u4"), ("off", "<u4"), ("len", "<u4"),
                          ("reserved", "<u4")])
assert RAW_PKT_DTYPE.itemsize == 24


class lkf_stream_srtp(C.Structure):
    _fields_ = [("s_l", C.c_uint64), ("mask", C.c_uint64), ("started", C.c_uint32), ("transport", C.c_int32),
                ("accepted", C.c_uint64), ("auth_failures", C.c_uint64), ("replays", C.c_uint64),
                ("malformed", C.c_uint64)]

    def as_tuple(self):
        return tuple(getattr(self, n) for n, _ in self._fields_)


assert C.sizeof(lkf_stream_srtp) == 56


# SRTCP (lkf_srtcp_unprotect / lkf_rtcp_ingest_unprotected / lkf_srtcp_protect)
LKF_SRTCP_SSRCS = 16
(LKF_SRTCP_RX_OK, LKF_SRTCP_RX_MALFORMED, LKF_SRTCP_RX_REPLAY_OLD, LKF_SRTCP_RX_REPLAY_DUP, LKF_SRTCP_RX_AUTH,
 LKF_SRTCP_RX_UNENCRYPTED, LKF_SRTCP_RX_NO_SLOT) = range(7)


class lkf_srtcp_raw(C.Structure):
    _fields_ = [("transport", C.c_int32), ("off", C.c_uint32), ("len", C.c_uint32)]


class lkf_srtcp_rx_result(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("ssrc", "index", "status", "len")]


class lkf_rtcp_entry(C.Structure):
    _fields_ = [("dt", C.c_int32), ("dgram", C.c_uint32)]


# RTCP demultiplexing (lkf_rtcp_demux / lkf_rtcp_demux_unprotected)
LKF_RTCP_DMX_OK, LKF_RTCP_DMX_EMPTY, LKF_RTCP_DMX_MALFORMED = range(3)


class lkf_rtcp_dmx_result(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("status", "dests", "unrouted", "entries")]


class lkf_srtcp_tx_result(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("ssrc", "index", "off", "len")]


class lkf_transport_srtcp(C.Structure):
    _fields_ = ([(f, C.c_uint32 * LKF_SRTCP_SSRCS) for f in ("in_use", "ssrc", "latest")]
                + [("mask", C.c_uint64 * LKF_SRTCP_SSRCS)]
                + [(f, C.c_uint64) for f in ("accepted", "auth_failures", "replays", "malformed", "unencrypted",
                                             "no_slot")])

    def as_tuple(self):
        """(slots [(in_use, ssrc, latest, mask)] * 16, (the six counters))."""
        slots = [(self.in_use[k], self.ssrc[k], self.latest[k], self.mask[k]) for k in range(LKF_SRTCP_SSRCS)]
        return slots, (self.accepted, self.auth_failures, self.replays, self.malformed, self.unencrypted,
                       self.no_slot)


SRTCP_RAW_DTYPE = np.dtype([("transport", "<i4"), ("off", "<u4"), ("len", "<u4")])
SRTCP_RX_RESULT_DTYPE = np.dtype([(f, "<u4") for f in ("ssrc", "index", "status", "len")])
RTCP_ENTRY_DTYPE = np.dtype([("dt", "<i4"), ("dgram", "<u4")])
SRTCP_TX_RESULT_DTYPE = np.dtype([(f, "<u4") for f in ("ssrc", "index", "off", "len")])
assert C.sizeof(lkf_srtcp_raw) == 12 == SRTCP_RAW_DTYPE.itemsize
assert C.sizeof(lkf_srtcp_rx_result) == 16 == SRTCP_RX_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_rtcp_entry) == 8 == RTCP_ENTRY_DTYPE.itemsize
RTCP_DMX_RESULT_DTYPE = np.dtype([(f, "<u4") for f in ("status", "dests", "unrouted", "entries")])
assert C.sizeof(lkf_rtcp_dmx_result) == 16 == RTCP_DMX_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_srtcp_tx_result) == 16 == SRTCP_TX_RESULT_DTYPE.itemsize
assert C.sizeof(lkf_transport_srtcp) == 368


class lkf_seq_meta(C.Structure):
    _fields_ = [
        ("ext_sn", C.c_uint64),
        ("ext_ts", C.c_uint64),
        ("source_sn", C.c_uint16),
        ("target_sn", C.c_uint16),
        ("timestamp", C.c_uint32),
        ("last_nack", C.c_uint32),
        ("marker", C.c_uint8),
        ("nacked", C.c_uint8),
        ("layer", C.c_int8),
        ("codec_len", C.c_uint8),
        ("codec", C.c_uint8 * 8),
    ]


class lkfs_cfg(C.Structure):
    _fields_ = [
        ("config", C.c_int32),
        ("seed", C.c_uint64),
        ("duration_s", C.c_double),
        ("batch_s", C.c_double),
        ("rooms", C.c_uint32),
        ("participants", C.c_uint32),
        ("room_base", C.c_uint32),
        ("loss", C.c_double),
        ("reorder", C.c_double),
        ("with_events", C.c_int32),
        ("has_callbacks", C.c_int32),
        ("svc_dd", C.c_int32),
        ("h264", C.c_int32),
        ("twcc", C.c_int32),
        ("room_ids", C.POINTER(C.c_uint32)),
    ]


class lkfs_event(C.Structure):
    _fields_ = [
        ("dt", C.c_int32),
        ("op", C.c_int32),
        ("a", C.c_int64 * 4),
        ("at_pkt", C.c_uint32),
        ("pad", C.c_uint32),
    ]


LKF_AT_PKT, LKF_AT_DATAGRAM, LKF_AT_ARRIVAL_NS = 0, 1, 2  # lkf_at_kind: how a control op names its position
LKF_AT_END = 0xFFFFFFFF  # the ExtPacket index that means "at batch end"


class lkf_ctl_event_key(C.Structure):  # lkf_ctl_batch_key: an op with its position as a key of `kind`
    _fields_ = [
        ("dt", C.c_int32),
        ("op", C.c_int32),
        ("a", C.c_int64 * 4),
        ("key", C.c_int64),
        ("kind", C.c_int32),
        ("pad", C.c_uint32),
    ]


assert C.sizeof(lkf_ctl_event_key) == 56, C.sizeof(lkf_ctl_event_key)
assert C.sizeof(lkf_pkt) == 64, C.sizeof(lkf_pkt)
assert C.sizeof(lkf_pkt_dd) == 32, C.sizeof(lkf_pkt_dd)
assert C.sizeof(lkf_track_params) == 64, C.sizeof(lkf_track_params)
assert C.sizeof(lkf_out) == 40, C.sizeof(lkf_out)

LKF_OUT_SWITCHING, LKF_OUT_RESUMING, LKF_OUT_KEYFRAME, LKF_OUT_MARKER = 0x01, 0x02, 0x04, 0x08  # lkf_out.flags
OUT_DTYPE = np.dtype(
    [("ext_sn", "<u8"), ("ext_ts", "<u8"), ("out_off", "<u8"), ("dt", "<u4"), ("pkt", "<u4"),
     ("out_len", "<u2"), ("flags", "u1"), ("layer", "i1"), ("reserved", "<u4")]
)
assert OUT_DTYPE.itemsize == 40
PRE_DTYPE = np.dtype(
    [("ext_sn", "<u8"), ("ext_ts", "<u8"), ("pre_off", "<u8"), ("dt", "<u4"), ("pkt", "<u4"),
     ("out_len", "<u2"), ("flags", "u1"), ("layer", "i1"), ("pre_len", "<u2"), ("tail_len", "<u2"),
     ("tail_src", "<u4"), ("reserved", "<u4")]
)
assert C.sizeof(lkf_pre) == 48 == PRE_DTYPE.itemsize, (C.sizeof(lkf_pre), PRE_DTYPE.itemsize)


def _bind(lib, name, restype, argtypes):
    fn = getattr(lib, name)
    fn.restype = restype
    fn.argtypes = argtypes
    return fn


P = C.POINTER


def bind_engine_api(lib, prefix):
    """Binds the lkf_* (engine) or orc_* (oracle) entry points of `lib`."""
    e = C.c_void_p
    api = {}
    api["add_track"] = _bind(lib, prefix + "add_track", C.c_int32, [e, P(lkf_track_params)])
    api["add_downtrack"] = _bind(lib, prefix + "add_downtrack", C.c_int32, [e, P(lkf_downtrack_params)])
    api["remove_downtrack"] = _bind(lib, prefix + "remove_downtrack", C.c_int, [e, C.c_int32])
    api["remove_track"] = _bind(lib, prefix + "remove_track", C.c_int, [e, C.c_int32])
    api["set_layer_offsets"] = _bind(lib, prefix + "set_layer_offsets", C.c_int, [e, C.c_int32, P(C.c_uint32)])
    api["set_layer_offsets_at"] = _bind(lib, prefix + "set_layer_offsets_at", C.c_int,
                                        [e, C.c_int32, P(C.c_uint32), C.c_uint32])
    api["sender_report"] = _bind(lib, prefix + "sender_report", C.c_int,
                                 [e, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_uint32])
    api["ctl"] = _bind(lib, prefix + "ctl", C.c_int,
                       [e, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32])
    api["ctl_batch"] = _bind(lib, prefix + "ctl_batch", C.c_int, [e, C.c_void_p, C.c_uint32])
    if hasattr(lib, prefix + "ctl_key"):  # engine only: positions by datagram index or arrival time (lkf_at_kind)
        api["ctl_key"] = _bind(lib, prefix + "ctl_key", C.c_int,
                               [e, C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int32,
                                C.c_int64])
        api["ctl_batch_key"] = _bind(lib, prefix + "ctl_batch_key", C.c_int, [e, C.c_void_p, C.c_uint32])
        api["sender_report_key"] = _bind(lib, prefix + "sender_report_key", C.c_int,
                                         [e, C.c_int32, C.c_int32, C.c_uint64, C.c_uint32, C.c_int32, C.c_int64])
        api["set_layer_offsets_key"] = _bind(lib, prefix + "set_layer_offsets_key", C.c_int,
                                             [e, C.c_int32, P(C.c_uint32), C.c_int32, C.c_int64])
    api["get_stats"] = _bind(lib, prefix + "get_stats", C.c_int, [e, P(lkf_stats)])
    if hasattr(lib, prefix + "last_error"):
        api["last_error"] = _bind(lib, prefix + "last_error", C.c_char_p, [e])
    api["drain"] = _bind(lib, prefix + "drain", C.c_int,
                         [e, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_uint64)])
    if hasattr(lib, prefix + "set_egress"):  # engine only: prefix egress (the oracle emits whole wire packets)
        api["set_egress"] = _bind(lib, prefix + "set_egress", C.c_int, [e, C.c_int])
        api["drain_prefix"] = _bind(lib, prefix + "drain_prefix", C.c_int,
                                    [e, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, P(C.c_uint64), P(C.c_uint64)])
        api["drain_prefix_run"] = _bind(lib, prefix + "drain_prefix_run", C.c_int,
                                        [e, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                         P(C.c_uint64), P(C.c_uint64)])
        api["output_prefix_device"] = _bind(lib, prefix + "output_prefix_device", C.c_int,
                                            [e, P(C.c_void_p), P(C.c_uint64), P(C.c_void_p), P(C.c_uint64)])
    api["get_state"] = _bind(lib, prefix + "get_state", C.c_int, [e, C.c_int32, P(lkf_fwd_state)])
    api["seed_state"] = _bind(lib, prefix + "seed_state", C.c_int, [e, C.c_int32, P(lkf_fwd_state)])
    api["seq_lookup"] = _bind(lib, prefix + "seq_lookup", C.c_int,
                              [e, C.c_int32, P(C.c_uint16), C.c_uint32, C.c_int64, P(lkf_seq_meta), P(C.c_uint32)])
    api["add_stream"] = _bind(lib, prefix + "add_stream", C.c_int32, [e, P(lkf_stream_params)])
    api["ingest"] = _bind(lib, prefix + "ingest", C.c_int, [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64])
    if hasattr(lib, prefix + "ingest_device"):  # engine only (the oracle is host-side)
        api["ingest_device"] = _bind(lib, prefix + "ingest_device", C.c_int,
                                     [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64])
    api["ingest_twcc"] = _bind(lib, prefix + "ingest_twcc", C.c_int, [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["ingest_flows"] = _bind(lib, prefix + "ingest_flows", C.c_int, [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["ingested"] = _bind(lib, prefix + "ingested", C.c_int, [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["ingested_dd"] = _bind(lib, prefix + "ingested_dd", C.c_int, [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["submit_dd"] = _bind(lib, prefix + "submit_dd", C.c_int, [e, C.c_void_p, C.c_uint32])
    if hasattr(lib, prefix + "submit_dd_device"):  # engine only
        api["submit_dd_device"] = _bind(lib, prefix + "submit_dd_device", C.c_int, [e, C.c_void_p, C.c_uint32])
    if hasattr(lib, prefix + "speakers_enqueue"):
        api["speakers_enqueue"] = _bind(lib, prefix + "speakers_enqueue", C.c_int, [e, C.c_int64])
    if hasattr(lib, prefix + "room_summaries_enqueue"):  # engine only (device records)
        api["room_summaries_enqueue"] = _bind(lib, prefix + "room_summaries_enqueue", C.c_int,
                                              [e, C.c_int64, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.c_void_p, C.c_uint32, C.c_void_p])
    api["stream_stats_get"] = _bind(lib, prefix + "stream_stats_get", C.c_int, [e, C.c_int32, P(lkf_stream_stats)])
    api["ingest_nacks"] = _bind(lib, prefix + "ingest_nacks", C.c_int,
                                [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, P(C.c_uint32), P(C.c_uint32)])
    api["stream_set_rtt"] = _bind(lib, prefix + "stream_set_rtt", C.c_int, [e, C.c_int32, C.c_uint32])
    api["speakers"] = _bind(lib, prefix + "speakers", C.c_int, [e, C.c_int64, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["downtrack_summaries"] = _bind(lib, prefix + "downtrack_summaries", C.c_int,
                                       [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["rtx_lookup"] = _bind(lib, prefix + "rtx_lookup", C.c_int,
                              [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    api["rtx_emit"] = _bind(lib, prefix + "rtx_emit", C.c_int,
                            [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                             C.c_uint64, P(C.c_uint32), P(C.c_uint64)])
    api["rtx_emit_bucket"] = _bind(lib, prefix + "rtx_emit_bucket", C.c_int,
                                   [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, P(C.c_uint32),
                                    P(C.c_uint64)])
    api["add_transport"] = _bind(lib, prefix + "add_transport", C.c_int32, [e, P(lkf_transport_params)])
    api["set_downtrack_transport"] = _bind(lib, prefix + "set_downtrack_transport", C.c_int, [e, C.c_int32, C.c_int32])
    api["protect"] = _bind(lib, prefix + "protect", C.c_int, [e, C.c_int64])
    api["drain_protected"] = _bind(lib, prefix + "drain_protected", C.c_int, [e, C.c_void_p, C.c_uint64, P(C.c_uint64)])
    if hasattr(lib, prefix + "unprotect_device"):  # engine only: SRTP unprotect in front of ingress
        api["set_stream_transport"] = _bind(lib, prefix + "set_stream_transport", C.c_int, [e, C.c_int32, C.c_int32])
        api["unprotect_device"] = _bind(lib, prefix + "unprotect_device", C.c_int,
                                        [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p])
        api["ingest_srtp"] = _bind(lib, prefix + "ingest_srtp", C.c_int,
                                   [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64])
        api["unprotect_results"] = _bind(lib, prefix + "unprotect_results", C.c_int,
                                         [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
        api["stream_srtp_get"] = _bind(lib, prefix + "stream_srtp_get", C.c_int, [e, C.c_int32, P(lkf_stream_srtp)])
        api["unprotect_timing_window"] = _bind(lib, prefix + "unprotect_timing_window", C.c_int,
                                               [e, C.c_uint32, P(C.c_float)])
    if hasattr(lib, prefix + "protect_timing_window"):
        api["protect_timing_window"] = _bind(lib, prefix + "protect_timing_window", C.c_int,
                                             [e, C.c_uint32, P(C.c_float)])
    if not hasattr(lib, prefix + "padding"):  # (an older build, e.g. an A/B baseline library)
        return api
    api["padding"] = _bind(lib, prefix + "padding", C.c_int,
                           [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                            P(C.c_uint32), P(C.c_uint64), C.c_void_p])
    if hasattr(lib, prefix + "add_stream_tracker"):
        api["add_stream_tracker"] = _bind(lib, prefix + "add_stream_tracker", C.c_int32,
                                          [e, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32])
        api["stream_tracker_ctl"] = _bind(lib, prefix + "stream_tracker_ctl", C.c_int, [e, C.c_int32, C.c_int32, C.c_int32])
        api["stream_trackers_tick"] = _bind(lib, prefix + "stream_trackers_tick", C.c_int,
                                            [e, C.c_void_p, C.c_uint32, C.c_int, C.c_int64, C.c_void_p])
    if hasattr(lib, prefix + "add_stream_tracker_frame"):
        api["add_stream_tracker_frame"] = _bind(lib, prefix + "add_stream_tracker_frame", C.c_int32,
                                                [e, C.c_int32, C.c_int32, C.c_uint32, C.c_double])
        api["stream_trackers_tick_at"] = _bind(lib, prefix + "stream_trackers_tick_at", C.c_int,
                                               [e, C.c_void_p, C.c_uint32, C.c_int, C.c_int64, C.c_int64, C.c_void_p])
    if hasattr(lib, prefix + "red_encode"):
        for nm in ("red_encode", "red_decode"):
            api[nm] = _bind(lib, prefix + nm, C.c_int,
                            [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                             C.c_uint32, C.c_void_p, C.c_uint64, P(C.c_uint32), P(C.c_uint64)])
    if hasattr(lib, prefix + "allocate_optimal"):
        api["allocate_optimal"] = _bind(lib, prefix + "allocate_optimal", C.c_int,
                                        [e, C.c_void_p, C.c_uint32, C.c_void_p])
    if hasattr(lib, prefix + "pause"):
        api["allocate_next_higher"] = _bind(lib, prefix + "allocate_next_higher", C.c_int,
                                            [e, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p])
        api["next_higher_transition"] = _bind(lib, prefix + "next_higher_transition", C.c_int,
                                              [e, C.c_void_p, C.c_uint32, C.c_void_p])
        api["pause"] = _bind(lib, prefix + "pause", C.c_int, [e, C.c_void_p, C.c_uint32, C.c_void_p])
    if hasattr(lib, prefix + "add_stream_tracker_dd"):
        api["add_stream_tracker_dd"] = _bind(lib, prefix + "add_stream_tracker_dd", C.c_int32, [e, C.c_int32])
        api["dd_tracker_ctl"] = _bind(lib, prefix + "dd_tracker_ctl", C.c_int, [e, C.c_int32, C.c_int32, C.c_int32])
        api["dd_trackers_tick"] = _bind(lib, prefix + "dd_trackers_tick", C.c_int,
                                        [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p])
    if hasattr(lib, prefix + "provisional_prepare"):
        api["provisional_prepare"] = _bind(lib, prefix + "provisional_prepare", C.c_int, [e, C.c_void_p, C.c_uint32])
        api["provisional_reset"] = _bind(lib, prefix + "provisional_reset", C.c_int, [e, C.c_void_p, C.c_uint32])
        for nm in ("provisional_allocate", "provisional_cooperative", "provisional_best_weighted",
                   "provisional_commit"):
            api[nm] = _bind(lib, prefix + nm, C.c_int, [e, C.c_void_p, C.c_uint32, C.c_void_p])
        api["allocate_all"] = _bind(lib, prefix + "allocate_all", C.c_int,
                                    [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p])
    if hasattr(lib, prefix + "sender_stats_get"):
        api["sender_stats_get"] = _bind(lib, prefix + "sender_stats_get", C.c_int, [e, C.c_int32, C.c_void_p])
        api["sender_sninfo"] = _bind(lib, prefix + "sender_sninfo", C.c_int, [e, C.c_int32, C.c_uint64, P(C.c_uint32)])
        api["sender_stats_seed"] = _bind(lib, prefix + "sender_stats_seed", C.c_int, [e, C.c_int32, C.c_int32])
    if hasattr(lib, prefix + "rtcp_feedback"):  # engine only: the DownTrack RTCP loop
        api["rtcp_feedback"] = _bind(lib, prefix + "rtcp_feedback", C.c_int,
                                     [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p])
        api["rtcp_sender_reports"] = _bind(lib, prefix + "rtcp_sender_reports", C.c_int,
                                           [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p])
        api["sender_delta_info"] = _bind(lib, prefix + "sender_delta_info", C.c_int,
                                         [e, C.c_void_p, C.c_uint32, C.c_void_p])
        api["sender_rtcp_get"] = _bind(lib, prefix + "sender_rtcp_get", C.c_int, [e, C.c_int32, C.c_void_p])
    if hasattr(lib, prefix + "rtcp_ingest"):  # engine only: RTCP ingress
        api["rtcp_ingest"] = _bind(lib, prefix + "rtcp_ingest", C.c_int,
                                   [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_uint32, P(C.c_uint32), C.c_void_p, C.c_uint32,
                                    P(C.c_uint32), P(C.c_uint32)])
        api["rtcp_ingested_nacks"] = _bind(lib, prefix + "rtcp_ingested_nacks", C.c_int,
                                           [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
        api["rtx_lookup_ingested"] = _bind(lib, prefix + "rtx_lookup_ingested", C.c_int,
                                           [e, C.c_int64, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    if hasattr(lib, prefix + "srtcp_unprotect"):  # engine only: SRTCP
        api["srtcp_unprotect"] = _bind(lib, prefix + "srtcp_unprotect", C.c_int,
                                       [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p])
        api["rtcp_ingest_unprotected"] = _bind(lib, prefix + "rtcp_ingest_unprotected", C.c_int,
                                               [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_uint32, P(C.c_uint32), C.c_void_p, C.c_uint32,
                                                P(C.c_uint32), P(C.c_uint32)])
        api["transport_srtcp_get"] = _bind(lib, prefix + "transport_srtcp_get", C.c_int,
                                           [e, C.c_int32, P(lkf_transport_srtcp)])
        api["srtcp_reset"] = _bind(lib, prefix + "srtcp_reset", C.c_int, [e, C.c_int32])
        api["srtcp_protect"] = _bind(lib, prefix + "srtcp_protect", C.c_int,
                                     [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64,
                                      C.c_void_p, P(C.c_uint64)])
        api["srtcp_tx_index"] = _bind(lib, prefix + "srtcp_tx_index", C.c_int,
                                      [e, C.c_int32, C.c_uint32, P(C.c_uint32)])
    if hasattr(lib, prefix + "rtcp_demux"):  # engine only: RTCP demultiplexing
        api["set_downtrack_rtcp_transport"] = _bind(lib, prefix + "set_downtrack_rtcp_transport", C.c_int,
                                                    [e, C.c_int32, C.c_int32])
        api["rtcp_demux_unprotected"] = _bind(lib, prefix + "rtcp_demux_unprotected", C.c_int,
                                              [e, C.c_void_p, C.c_void_p, C.c_uint32, P(C.c_uint32)])
        api["rtcp_demux"] = _bind(lib, prefix + "rtcp_demux", C.c_int,
                                  [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                   C.c_uint32, P(C.c_uint32)])
    if hasattr(lib, prefix + "stream_sender_reports"):  # engine only: the publisher RTCP loop
        api["stream_sender_reports"] = _bind(lib, prefix + "stream_sender_reports", C.c_int,
                                             [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p])
        api["stream_receiver_reports"] = _bind(lib, prefix + "stream_receiver_reports", C.c_int,
                                               [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p])
        api["stream_rtcp_ingest"] = _bind(lib, prefix + "stream_rtcp_ingest", C.c_int,
                                          [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int64, C.c_void_p])
        api["stream_rtcp_ingest_unprotected"] = _bind(lib, prefix + "stream_rtcp_ingest_unprotected", C.c_int,
                                                      [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p])
        api["ingest_nacks_wire"] = _bind(lib, prefix + "ingest_nacks_wire", C.c_int,
                                         [e, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, P(C.c_uint32),
                                          P(C.c_uint64)])
        api["stream_rtcp_get"] = _bind(lib, prefix + "stream_rtcp_get", C.c_int, [e, C.c_int32, C.c_void_p])
    if hasattr(lib, prefix + "stream_fps_enable"):  # engine only: the ingress frame-rate calculators
        api["stream_fps_enable"] = _bind(lib, prefix + "stream_fps_enable", C.c_int, [e, C.c_int32])
        api["stream_fps_get"] = _bind(lib, prefix + "stream_fps_get", C.c_int, [e, C.c_int32, P(lkf_stream_fps)])
        api["ingest_fps_changed"] = _bind(lib, prefix + "ingest_fps_changed", C.c_int,
                                          [e, C.c_void_p, C.c_uint32, P(C.c_uint32)])
    if hasattr(lib, prefix + "stream_fps_enable_dd"):  # ... and the dependency-descriptor calculator
        api["stream_fps_enable_dd"] = _bind(lib, prefix + "stream_fps_enable_dd", C.c_int, [e, C.c_int32])
        api["stream_fps_dd_get"] = _bind(lib, prefix + "stream_fps_dd_get", C.c_int, [e, C.c_int32, P(lkf_fps_dd)])
    api["blank_frames"] = _bind(lib, prefix + "blank_frames", C.c_int,
                                [e, C.c_void_p, C.c_uint32, C.c_int64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64,
                                 P(C.c_uint32), P(C.c_uint64)])
    return api


def load_synth(path=None):
    path = path or os.path.join(LIBDIR, "liblkfsynth.so")
    lib = C.CDLL(path)
    t = C.c_void_p
    _bind(lib, "lkfs_generate", t, [P(lkfs_cfg)])
    _bind(lib, "lkfs_free", None, [t])
    _bind(lib, "lkfs_num_tracks", C.c_uint32, [t])
    _bind(lib, "lkfs_num_downtracks", C.c_uint32, [t])
    _bind(lib, "lkfs_tracks", P(lkf_track_params), [t])
    _bind(lib, "lkfs_downtracks", P(lkf_downtrack_params), [t])
    _bind(lib, "lkfs_num_batches", C.c_uint32, [t])
    _bind(lib, "lkfs_batch", C.c_int,
          [t, C.c_uint32, P(P(lkf_pkt)), P(C.c_uint32), P(P(C.c_uint8)), P(C.c_uint64)])
    _bind(lib, "lkfs_batch_events", C.c_int, [t, C.c_uint32, P(P(lkfs_event)), P(C.c_uint32)])
    _bind(lib, "lkfs_total_pkts", C.c_uint64, [t])
    _bind(lib, "lkfs_total_arena", C.c_uint64, [t])
    _bind(lib, "lkfs_max_batch_pkts", C.c_uint32, [t])
    _bind(lib, "lkfs_max_batch_arena", C.c_uint64, [t])
    _bind(lib, "lkfs_max_batch_tuples", C.c_uint64, [t])
    _bind(lib, "lkfs_max_batch_out_bytes", C.c_uint64, [t])
    _bind(lib, "lkfs_num_streams", C.c_uint32, [t])
    _bind(lib, "lkfs_streams", P(lkf_stream_params), [t])
    _bind(lib, "lkfs_batch_raw", C.c_int, [t, C.c_uint32, P(P(lkf_raw_pkt)), P(C.c_uint32)])
    _bind(lib, "lkfs_batch_dd", C.c_int, [t, C.c_uint32, P(P(lkf_pkt_dd)), P(C.c_uint32)])
    return lib
