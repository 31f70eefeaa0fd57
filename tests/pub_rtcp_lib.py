"""The publisher RTCP loop's checker: PyStreamRtcp, an independent restatement
of the RTCP half of buffer.RTPStatsReceiver on plain Python ints.

Written from rtpstats_receiver.go:243-396 (SetRtcpSenderReportData,
GetRtcpReceptionReport), rtpstats_base.go:469-515 and :812-914
(maybeAdjustFirstPacketTime, getAndResetSnapshot), mediatrack.go:193-208 and
the text of include/lkfwd.h ("the publisher RTCP loop"), not from
pub_rtcp_device.h.  float32 rounding goes through struct.pack("<f"); bytes are
built and read with struct.  The per-packet counters are not this class's: it
reads them from `hot`, a dict the caller keeps (the unit program's script, or
lkf_stream_stats_get on the GPU):
    init, sn_start, ext_highest_sn, ts_start, packets_lost, jitter (float),
    first_time (written back by the first-packet-time adjustment)
"""
import struct

from tests.rtcp_lib import M32, M64, go_div, ntp_to_unix, s64, seconds

SSR_IGNORED_UNINIT, SSR_ANACHRONOUS, SSR_CLOCK_SKEW, SSR_RESET_FIRST = 1, 2, 4, 8
SSR_FIRST_TIME_ADJUSTED, SSR_ADJUST_TOO_BIG, SSR_CLOSED = 0x10, 0x20, 0x40
SRR_VALID = 1
IN_OK, IN_MALFORMED = 0, 1
WINDOW_NS = 2 * 60 * 10**9
THRESHOLD_NS = 5 * 60 * 10**9
RR_FIELDS = ("flags", "ssrc", "fraction_lost", "total_lost", "last_sequence_number", "jitter", "last_sender_report",
             "delay")


def f32(x):
    """Rounds a Python float (or int) to float32 and back."""
    return struct.unpack("<f", struct.pack("<f", x))[0]


def go_i64(v):
    """int64(float64) as amd64 Go converts it (include/lkfwd.h)."""
    if v != v or not (-(2.0 ** 63) <= v < 2.0 ** 63):
        return -(1 << 63)
    return int(v)


def go_u32(v):
    """uint32(float64): the low 32 bits of the value truncated to int64."""
    return go_i64(v) & M32


def go_u8_f32(v):
    """uint8(float32): the low 8 bits of the value truncated to int32."""
    if v != v or not (-(2.0 ** 31) <= v < 2.0 ** 31):
        return 0  # 0x80000000
    return int(v) & 0xFF


class PyStreamRtcp:
    def __init__(self, clock, ssrc):
        self.clock, self.ssrc = clock, ssrc
        self.closed = False
        self.sr_first = self.sr_newest = None  # (ntp, rtp_ext, at)
        self.snap = None  # (start_time, ext_start_sn, packets_lost)
        self.started, self.start_time = 0, 0
        self.clock_skew_count = self.out_of_order_sr_count = 0

    def _capture(self, hot):
        if not self.started and hot["init"]:
            self.started, self.start_time = 1, hot["first_time"]

    # maybeAdjustFirstPacketTime
    def _adjust(self, hot, ts, now):
        if now - self.start_time > WINDOW_NS:
            return 0
        diff = (ts - hot["ts_start"]) & M32
        if diff >= 1 << 31:  # int32 < 0
            return 0
        dur = go_i64(float(diff) / float(self.clock) * 1e9)
        first = s64(now - dur)
        if first < hot["first_time"]:
            if hot["first_time"] - first > THRESHOLD_NS:
                return SSR_ADJUST_TOO_BIG
            hot["first_time"] = first
            return SSR_FIRST_TIME_ADJUSTED
        return 0

    def sender_report(self, hot, rtp, ntp, now):
        """SetSenderReportData(rtp, ntp) at `now` -> (flags, stored ntp, stored rtp_ext)."""
        if self.closed:
            return SSR_CLOSED, 0, 0
        if not hot["init"]:
            return SSR_IGNORED_UNINIT, 0, 0
        self._capture(hot)
        new = self.sr_newest
        if new is not None and new[0] > ntp:
            return SSR_ANACHRONOUS, 0, 0
        cycles = 0
        if new is not None:
            cycles = new[1] & 0xFFFFFFFF00000000
            last = new[1] & M32
            if (rtp - last) & M32 < 1 << 31 and rtp < last:
                cycles += 1 << 32
        ext = (rtp + cycles) & M64
        flags = self._adjust(hot, rtp, now)
        if new is not None:
            t = ntp_to_unix(ntp)

            def rate(ref):
                dt = seconds(s64(t - ntp_to_unix(ref[0])))
                ticks = float((ext - ref[1]) & M64)  # (an int rounds to the nearest double, as Go's conversion)
                if dt == 0.0:
                    r = float("nan") if ticks == 0.0 else float("inf")
                else:
                    r = ticks / dt
                return dt, r

            lim = 0.2 * float(self.clock)
            skew = False
            for ref in (new, self.sr_first):
                dt, r = rate(ref)
                skew = skew or (dt > 0.2 and abs(float(self.clock) - r) > lim)
            if skew:
                self.clock_skew_count += 1
                flags |= SSR_CLOCK_SKEW
            if ext < new[1]:
                self.out_of_order_sr_count += 1
                self.sr_first = None
                flags |= SSR_RESET_FIRST
        self.sr_newest = (ntp, ext, now)
        if self.sr_first is None:
            self.sr_first = self.sr_newest
        return flags, ntp, ext

    def reception_report(self, hot, proxy, now):
        """GetRtcpReceptionReport -> dict of RR_FIELDS (flags 0 and zeros: nil)."""
        nil = dict.fromkeys(RR_FIELDS, 0)
        if self.closed or not hot["init"]:
            return nil
        self._capture(hot)
        then = self.snap if self.snap is not None else (self.start_time, hot["sn_start"], 0)
        self.snap = (now, (hot["ext_highest_sn"] + 1) & M64, hot["packets_lost"])
        expected = (self.snap[1] - then[1]) & M64
        if expected > 65536 or expected == 0:
            return nil
        lost = (self.snap[2] - then[2]) & M32
        if lost >= 1 << 31:
            lost = 0
        rate = f32(f32(lost) / f32(expected))
        frac = max(go_u8_f32(f32(rate * 256.0)), proxy & 0xFF)
        lsr = dlsr = 0
        if self.sr_newest is not None:
            lsr = (self.sr_newest[0] >> 16) & M32
            if self.sr_newest[2] != 0:
                us = go_div(s64(now - self.sr_newest[2]), 1000)
                dlsr = go_div(s64(us * 65536), 1000000) & M32
        return dict(flags=SRR_VALID, ssrc=self.ssrc, fraction_lost=frac, total_lost=min(hot["packets_lost"], 0xFFFFFF),
                    last_sequence_number=self.snap[1] & M32, jitter=go_u32(hot["jitter"]), last_sender_report=lsr,
                    delay=dlsr)

    @staticmethod
    def wire(r):
        """rtcp.ReceiverReport{SSRC, [one report]}.Marshal() of a reception_report() dict: 32 bytes."""
        if not r["flags"] & SRR_VALID:
            return bytes(32)
        return struct.pack(">BBHIIIIIII", 0x81, 201, 7, r["ssrc"], r["ssrc"],
                           (r["fraction_lost"] << 24) | r["total_lost"], r["last_sequence_number"], r["jitter"],
                           r["last_sender_report"], r["delay"])

    @staticmethod
    def sender_reports_of(data):
        """The (rtp, ntp) of every sender report of a compound packet, or None when it is malformed: the
        framing and the size checks of include/lkfwd.h's RTCP ingress table."""
        if len(data) == 0:
            return None
        out, at = [], 0
        while at < len(data):
            left = data[at:]
            if len(left) < 4:
                return None
            b0, pt, length = struct.unpack(">BBH", left[:4])
            size = 4 * (length + 1)
            if b0 >> 6 != 2 or size > len(left):
                return None
            c = b0 & 31
            ok = {201: size >= 8 + 24 * c, 200: size >= 28 + 24 * c}.get(pt, True)
            if pt == 205:
                ok = size >= (12 if c == 1 else 20 if c == 15 else 0)
            if pt == 206:
                if c == 1:
                    ok = size >= 12
                elif c == 4:
                    ok = size >= 12 and (size - 12) % 8 == 0
                elif c == 15:
                    ok = size >= 20 and left[12:16] == b"REMB" and size >= 20 + 4 * left[16]
            if not ok:
                return None
            if pt == 200:
                ntp, rtp = struct.unpack(">QI", left[8:20])
                out.append((rtp, ntp))
            at += size
        return out

    def ingest(self, hot, data, now):
        """One rtcpReader.OnPacket(data) -> dict(status, n_sr, flags, ntp, rtp_ext)."""
        srs = self.sender_reports_of(bytes(data))
        res = dict(status=IN_MALFORMED, n_sr=0, flags=0, ntp=0, rtp_ext=0)
        if srs is None:
            return res
        res.update(status=IN_OK, n_sr=len(srs))
        for rtp, ntp in srs:
            fl, sntp, sext = self.sender_report(hot, rtp, ntp, now)
            res["flags"] |= fl
            if sntp or sext:
                res["ntp"], res["rtp_ext"] = sntp, sext
        return res

    def state(self, hot):
        """The words pub_rtcp_unit prints / lkf_stream_rtcp_get returns (engine_state below)."""
        st = dict(initialized=int(bool(hot["init"])), first_time=hot["first_time"], started=self.started,
                  start_time=self.start_time, snap_is_valid=int(self.snap is not None),
                  snap_start_time=self.snap[0] if self.snap else 0, snap_ext_start_sn=self.snap[1] if self.snap else 0,
                  snap_packets_lost=self.snap[2] if self.snap else 0, clock_skew_count=self.clock_skew_count,
                  out_of_order_sr_count=self.out_of_order_sr_count)
        for i, sr in enumerate((self.sr_first, self.sr_newest)):
            ntp, ext, at = sr if sr is not None else (0, 0, 0)
            st.update({"sr%d_valid" % i: int(sr is not None), "sr%d_ntp" % i: ntp, "sr%d_rtp_ext" % i: ext,
                       "sr%d_at" % i: at})
        return st


def engine_state(row, stats):
    """An abi.STREAM_RTCP_DTYPE row and the stream's lkf_stream_stats -> PyStreamRtcp.state()'s dict."""
    st = dict(initialized=int(stats.initialized), first_time=int(stats.first_time_ns), started=int(row["started"]),
              start_time=int(row["start_time_ns"]), snap_is_valid=int(row["snapshot_is_valid"]),
              snap_start_time=int(row["snapshot_start_time_ns"]), snap_ext_start_sn=int(row["snapshot_ext_start_sn"]),
              snap_packets_lost=int(row["snapshot_packets_lost"]), clock_skew_count=int(row["clock_skew_count"]),
              out_of_order_sr_count=int(row["out_of_order_sender_report_count"]))
    for i, k in enumerate(("sr_first", "sr_newest")):
        st.update({"sr%d_valid" % i: int(row[k]["valid"]), "sr%d_ntp" % i: int(row[k]["ntp"]),
                   "sr%d_rtp_ext" % i: int(row[k]["rtp_ext"]), "sr%d_at" % i: int(row[k]["at_ns"])})
    return st


def hot_of(stats):
    """The `hot` dict from an lkf_stream_stats (its ext_start_sn / ext_start_ts are the 16 / 32-bit starts)."""
    return dict(init=bool(stats.initialized), sn_start=int(stats.ext_start_sn), ext_highest_sn=int(stats.ext_highest_sn),
                ts_start=int(stats.ext_start_ts) & M32, packets_lost=int(stats.packets_lost), jitter=float(stats.jitter),
                first_time=int(stats.first_time_ns))
