"""PyRtcp — the checker of the DownTrack RTCP loop (rtcp_device.h,
rtcp_kernels.hip): a plain-Python restatement of the RTCP half of
buffer.RTPStatsSender, written from the reference (rtpstats_sender.go,
rtpstats_base.go) and from the three mediatransportutil definitions of
include/lkfwd.h, with Go's integer wrap-around and float64 arithmetic.

It sits on a PySender (tests/test_sender_cpu.py): the per-packet counters and
the snInfo ring come from replaying that restatement, so nothing here reads
what the engine computed.

  UpdateFromReceiverReport  rtpstats_sender.go:441-565 (no base snapshots)
  GetRtcpSenderReport       :596-714
  DeltaInfoSender           :723-808, getAndResetSenderSnapshot :832-848,
                            initSenderSnapshot :850-857, getSenderSnapshot :859-887
  getIntervalStats          :947-987
  getTotalPacketsPrimary    rtpstats_base.go:517-530
  UpdateNack/Pli/Fir        rtpstats_base.go:315-324, :351-364, :407-416

time.Now() is the call's now (Unix ns), the zero time is 0, startTime is the
PySender's first packet time, and there is one senderSnapshot which starts as
the zero value (DownTrack takes its id before the first packet).
"""
import math
import struct

import numpy as np

from tests import rtcp_wire_lib as W
from tests.test_sender_cpu import M64, SN_INFO, PySender, s64

M32 = (1 << 32) - 1
NTP_EPOCH_NS = 2208988800 * 10**9
FB_RTT_CHANGED, FB_IGNORED, FB_CACHE_OVERFLOW = 1, 2, 4
SR_VALID, SR_CLOCK_SKEW, SR_REPAIRED = 1, 2, 4
IS_FIELDS = ("packets", "bytes", "header_bytes", "packets_padding", "bytes_padding", "header_bytes_padding",
             "packets_lost", "packets_out_of_order", "packets_not_found", "frames")


def bits(x):
    """A float64's 64 bits."""
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def go_div(a, b):
    """Go's signed integer division (truncates toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def seconds(d):
    """time.Duration.Seconds."""
    sec = go_div(d, 10**9)
    nsec = d - sec * 10**9
    return float(sec) + float(nsec) / 1e9


def go_u64(v):
    """uint64(float64) as amd64 Go converts it."""
    if not (-(2.0 ** 63) < v < 2.0 ** 64):
        return 1 << 63
    if v < 2.0 ** 63:
        return int(v) & M64
    return int(v - 2.0 ** 63) ^ (1 << 63)


def to_ntp(unix_ns):
    """mediatransportutil.ToNtpTime (include/lkfwd.h)."""
    n = (unix_ns + NTP_EPOCH_NS) & M64
    sec = n // 10**9
    f = (n - sec * 10**9) << 32
    frac = f // 10**9 + (1 if f % 10**9 >= 5 * 10**8 else 0)
    return ((sec << 32) | frac) & M64


def ntp_duration(t):
    """NtpTime.Duration: ns since the NTP epoch."""
    sec = (t >> 32) * 10**9
    frac = (t & M32) * 10**9
    nsec = (frac >> 32) + (1 if frac & M32 >= 0x80000000 else 0)
    return s64(sec + nsec)


def ntp_to_unix(t):
    return s64(ntp_duration(t) - NTP_EPOCH_NS)


def get_rtt_ms(lsr, dlsr, last_sr_ntp, last_sent_at, now):
    """mediatransportutil.GetRttMs (include/lkfwd.h) -> rtt or None."""
    if lsr == 0:
        return None
    if last_sr_ntp != 0 and (last_sr_ntp >> 16) & M32 != lsr:
        return None
    now_ntp = to_ntp(s64(ntp_to_unix(last_sr_ntp) + (now - last_sent_at)))
    now32 = (now_ntp >> 16) & M32
    if now32 < (lsr + dlsr) & M32:
        return None
    return int(math.ceil(float((now32 - lsr - dlsr) & M32) * 1000.0 / 65536.0)) & M32


def rr_lsn(esn, ext_start_sn):
    """rr.LastSequenceNumber that acknowledges the DownTrack's sent extended SN `esn`."""
    return (esn - (ext_start_sn & ~0xFFFF)) & M32


def zero_snapshot():
    s = dict(is_valid=0, start_time=0, ext_start_sn=0, bytes=0, header_bytes=0, packets_padding=0, bytes_padding=0,
             header_bytes_padding=0, packets_duplicate=0, bytes_duplicate=0, header_bytes_duplicate=0,
             packets_out_of_order=0, packets_lost_feed=0, packets_lost=0, frames=0, nacks=0, plis=0, firs=0,
             max_rtt=0, max_jitter_feed=0.0, max_jitter=0.0, ext_last_rr_sn=0)
    s["interval_stats"] = dict.fromkeys(IS_FIELDS, 0)
    return s


class PyRtcp:
    def __init__(self, sender):
        assert isinstance(sender, PySender)
        self.s = sender
        self.ext_highest_sn_from_rr = 0
        self.last_rr_time = 0
        self.last_rr = (0, 0)  # LastSequenceNumber, TotalLost
        self.packets_lost_from_rr = 0
        self.jitter_from_rr = 0.0
        self.max_jitter_from_rr = 0.0
        self.end_time = 0
        self.rtt = self.max_rtt = 0
        self.nacks = self.plis = self.firs = 0
        self.sr_first = None  # (ntp, rtp_ext, at)
        self.sr_newest = None
        self.clock_skew_count = self.out_of_order_sr_count = self.cache_overflow_count = 0
        self.snap = zero_snapshot()

    # -- getIntervalStats: the found sequence numbers one by one, the others counted
    def interval_stats(self, start, end_ex, ehsn):
        is_ = dict.fromkeys(IS_FIELDS, 0)
        if end_ex < start:  # the divergence: about 2^64 iterations in Go, empty here
            return is_
        if s64(ehsn - start) < 0:  # every offset int64(ehsn - esn) is negative
            lo, hi = start, start
        else:
            lo, hi = max(start, ehsn - (SN_INFO - 1)), min(end_ex, ehsn + 1)
            if hi < lo:
                lo = hi = start
        is_["packets_not_found"] = (end_ex - start) - (hi - lo)
        for esn in range(lo, hi):
            off = s64(ehsn - esn)
            assert 0 <= off < SN_INFO
            size, hdr, flags = self.s.ring[esn & (SN_INFO - 1)]
            if size == 0:
                is_["packets_lost"] += 1
            elif flags & 2:
                is_["packets_padding"] += 1
                is_["bytes_padding"] += size
                is_["header_bytes_padding"] += hdr
            else:
                is_["packets"] += 1
                is_["bytes"] += size
                is_["header_bytes"] += hdr
                if flags & 4:
                    is_["packets_out_of_order"] += 1
            if flags & 1:
                is_["frames"] += 1
        return is_

    def receiver_report(self, now, lsn, total_lost, jitter, lsr, dlsr):
        """-> (rtt, LKF_FB_* flags)"""
        s = self.s
        if not s.init or self.end_time != 0:
            return 0, FB_IGNORED
        ext = ((self.ext_highest_sn_from_rr & 0xFFFFFFFF00000000) + lsn) & M64
        if self.last_rr_time != 0:
            if (lsn - self.last_rr[0]) & M32 < (1 << 31) and lsn < self.last_rr[0]:
                ext = (ext + (1 << 32)) & M64
        base = s.start_sn & 0xFFFFFFFFFFFF0000
        if (ext + base) & M64 < s.start_sn:
            return 0, FB_IGNORED
        if self.last_rr_time != 0 and self.ext_highest_sn_from_rr > ext:
            return 0, FB_IGNORED
        self.ext_highest_sn_from_rr = ext

        rtt, changed = 0, False
        if self.sr_newest is not None:
            r = get_rtt_ms(lsr, dlsr, self.sr_newest[0], self.sr_newest[2], now)
            if r is not None:
                rtt = r
                changed = rtt != self.rtt

        lost = ((self.packets_lost_from_rr & 0xFFFFFFFF00000000) + total_lost) & M64
        if (total_lost - self.last_rr[1]) & M32 < (1 << 31) and total_lost < self.last_rr[1]:
            lost = (lost + (1 << 32)) & M64
        self.packets_lost_from_rr = lost

        if changed:
            self.rtt = rtt
            self.max_rtt = max(self.max_rtt, rtt)
        self.jitter_from_rr = float(jitter)
        if self.jitter_from_rr > self.max_jitter_from_rr:
            self.max_jitter_from_rr = self.jitter_from_rr

        received = (self.ext_highest_sn_from_rr + base) & M64
        sn = self.snap
        if changed and rtt > sn["max_rtt"]:
            sn["max_rtt"] = rtt
        if self.jitter_from_rr > sn["max_jitter"]:
            sn["max_jitter"] = self.jitter_from_rr
        is_ = self.interval_stats((sn["ext_last_rr_sn"] + 1) & M64, (received + 1) & M64, s.high_sn)
        for k in IS_FIELDS:
            m = M32 if k == "frames" else M64
            sn["interval_stats"][k] = (sn["interval_stats"][k] + is_[k]) & m
        flags = FB_RTT_CHANGED if changed else 0
        if is_["packets_not_found"] != 0:
            self.cache_overflow_count += 1
            flags |= FB_CACHE_OVERFLOW
        sn["ext_last_rr_sn"] = received

        self.last_rr_time = now
        self.last_rr = (lsn, total_lost)
        self.last_interval = is_
        return rtt, flags

    def counts(self, nacks, plis, firs):
        if self.end_time != 0:
            return
        self.nacks = (self.nacks + nacks) & M32
        self.plis = (self.plis + plis) & M32
        self.firs = (self.firs + firs) & M32

    def stop(self):
        self.end_time = 1

    def total_packets_primary(self):
        s = self.s
        expected = (s.high_sn - s.start_sn + 1) & M64
        if s.c["packets_lost"] > expected:
            return 0
        seen = expected - s.c["packets_lost"]
        if s.c["packets_padding"] > seen:
            return 0
        return seen - s.c["packets_padding"]

    def sender_report(self, now_ns, calculated_clock_rate):
        """-> dict(flags, ntp, rtp, rtp_ext, packet_count, octet_count); flags 0: nil"""
        s = self.s
        if not s.init:
            return dict(flags=0, ntp=0, rtp=0, rtp_ext=0, packet_count=0, octet_count=0)
        since_first = s64(now_ns - s.first)
        now = s64(s.first + since_first)
        now_ntp = to_ntp(now)
        since_highest = s64(now - s.highest_t)
        rtp_ext = (s.high_ts + (go_div(s64(since_highest * s.cr), 10**9) & M64)) & M64
        flags = SR_VALID
        if calculated_clock_rate != 0:
            using_rate = (s.start_ts + go_u64(float(calculated_clock_rate) * seconds(since_first))) & M64
            if using_rate > rtp_ext:
                rtp_ext = using_rate
        if self.sr_newest is not None and rtp_ext >= self.sr_newest[1]:
            since_last = s64(ntp_duration(now_ntp) - ntp_duration(self.sr_newest[0]))
            diff = (rtp_ext - self.sr_newest[1]) & M64
            secs = seconds(since_last)
            if secs > 0.2:
                window = float(diff) / secs
                if abs(float(s.cr) - window) > 0.2 * float(s.cr):
                    self.clock_skew_count += 1
                    flags |= SR_CLOCK_SKEW
        if self.sr_newest is not None and rtp_ext < self.sr_newest[1]:
            self.out_of_order_sr_count += 1
            ntp_diff = s64(ntp_duration(now_ntp) - ntp_duration(self.sr_newest[0]))
            rtp_ext = (self.sr_newest[1] + go_u64(seconds(ntp_diff) * float(s.cr))) & M64
            flags |= SR_REPAIRED
        self.sr_newest = (now_ntp, rtp_ext, now)
        if self.sr_first is None:
            self.sr_first = self.sr_newest
        c = s.c
        return dict(flags=flags, ntp=now_ntp, rtp=rtp_ext & M32, rtp_ext=rtp_ext,
                    packet_count=(self.total_packets_primary() + c["packets_duplicate"] + c["packets_padding"]) & M32,
                    octet_count=(c["bytes"] + c["bytes_duplicate"] + c["bytes_padding"]) & M32)

    def sender_report_wire(self, rep, ssrc):
        if not rep["flags"] & SR_VALID:
            return bytes(28)
        return struct.pack(">BBHIQIII", 0x80, 200, 6, ssrc, rep["ntp"], rep["rtp"], rep["packet_count"],
                           rep["octet_count"])

    def delta(self):
        """DeltaInfoSender -> dict, or None for nil"""
        s = self.s
        if self.last_rr_time == 0:
            return None
        if not s.init:
            return None
        then = self.snap
        if not then["is_valid"]:
            then = zero_snapshot()
            then.update(is_valid=1, start_time=s.first, ext_start_sn=s.start_sn,
                        ext_last_rr_sn=(s.start_sn - 1) & M64)
        ti = then["interval_stats"]
        now = zero_snapshot()
        now.update(is_valid=1, start_time=self.last_rr_time, ext_start_sn=(then["ext_last_rr_sn"] + 1) & M64,
                   bytes=(then["bytes"] + ti["bytes"]) & M64,
                   header_bytes=(then["header_bytes"] + ti["header_bytes"]) & M64,
                   packets_padding=(then["packets_padding"] + ti["packets_padding"]) & M64,
                   bytes_padding=(then["bytes_padding"] + ti["bytes_padding"]) & M64,
                   header_bytes_padding=(then["header_bytes_padding"] + ti["header_bytes_padding"]) & M64,
                   packets_duplicate=s.c["packets_duplicate"], bytes_duplicate=s.c["bytes_duplicate"],
                   header_bytes_duplicate=s.c["header_bytes_duplicate"], packets_lost_feed=s.c["packets_lost"],
                   packets_out_of_order=(then["packets_out_of_order"] + ti["packets_out_of_order"]) & M64,
                   frames=(then["frames"] + ti["frames"]) & M32, nacks=self.nacks, plis=self.plis, firs=self.firs,
                   max_rtt=self.rtt, max_jitter_feed=s.jitter, max_jitter=self.jitter_from_rr,
                   ext_last_rr_sn=then["ext_last_rr_sn"])
        self.snap = now

        def i32(v):
            v &= M32
            return v - (1 << 32) if v >> 31 else v

        expected = (now["ext_start_sn"] - then["ext_start_sn"]) & M32
        if expected > 65536 or expected == 0:
            return None
        lost = (now["packets_lost"] - then["packets_lost"]) & M32
        if i32(lost) < 0:
            lost = 0
        lost_feed = (now["packets_lost_feed"] - then["packets_lost_feed"]) & M32
        if i32(lost_feed) < 0:
            lost_feed = 0
        if lost > expected:
            lost = expected
        max_jitter = then["max_jitter"] - then["max_jitter_feed"]
        if max_jitter < 0.0:
            max_jitter = 0.0
        padding = (now["packets_padding"] - then["packets_padding"]) & M32
        return dict(valid=1, start_time=then["start_time"], duration=s64(now["start_time"] - then["start_time"]),
                    packets=(expected - padding) & M32, bytes=(now["bytes"] - then["bytes"]) & M64,
                    header_bytes=(now["header_bytes"] - then["header_bytes"]) & M64,
                    packets_duplicate=(now["packets_duplicate"] - then["packets_duplicate"]) & M32,
                    bytes_duplicate=(now["bytes_duplicate"] - then["bytes_duplicate"]) & M64,
                    header_bytes_duplicate=(now["header_bytes_duplicate"] - then["header_bytes_duplicate"]) & M64,
                    packets_padding=padding, bytes_padding=(now["bytes_padding"] - then["bytes_padding"]) & M64,
                    header_bytes_padding=(now["header_bytes_padding"] - then["header_bytes_padding"]) & M64,
                    packets_lost=lost, packets_missing=lost_feed,
                    packets_out_of_order=(now["packets_out_of_order"] - then["packets_out_of_order"]) & M32,
                    frames=(now["frames"] - then["frames"]) & M32, rtt_max=then["max_rtt"],
                    jitter_max=bits(max_jitter / float(s.cr) * 1e6), nacks=(now["nacks"] - then["nacks"]) & M32,
                    plis=(now["plis"] - then["plis"]) & M32, firs=(now["firs"] - then["firs"]) & M32)

    def seed_from(self, other):
        """RTPStatsSender.Seed's RTCP half (rtpstats_sender.go:173-201, rtpstats_base.go:206-279)."""
        for k in ("ext_highest_sn_from_rr", "last_rr_time", "last_rr", "packets_lost_from_rr", "jitter_from_rr",
                  "max_jitter_from_rr", "rtt", "max_rtt", "nacks", "plis", "firs", "sr_first", "sr_newest"):
            setattr(self, k, getattr(other, k))
        self.snap = dict(other.snap, interval_stats=dict(other.snap["interval_stats"]))

    def state(self):
        """The RTCP state as integers (doubles as bits), keyed as rtcp_unit --replay prints it."""
        d = dict(ext_highest_sn_from_rr=self.ext_highest_sn_from_rr, last_rr_time=self.last_rr_time,
                 packets_lost_from_rr=self.packets_lost_from_rr, jitter_from_rr=bits(self.jitter_from_rr),
                 max_jitter_from_rr=bits(self.max_jitter_from_rr), end_time=self.end_time,
                 last_rr_lsn=self.last_rr[0], last_rr_total_lost=self.last_rr[1], rtt=self.rtt, max_rtt=self.max_rtt,
                 nacks=self.nacks, plis=self.plis, firs=self.firs, clock_skew_count=self.clock_skew_count,
                 out_of_order_sr_count=self.out_of_order_sr_count, cache_overflow_count=self.cache_overflow_count)
        for i, sr in enumerate((self.sr_first, self.sr_newest)):
            v = sr or (0, 0, 0)
            d.update({"sr%d_valid" % i: 1 if sr else 0, "sr%d_ntp" % i: v[0], "sr%d_rtp_ext" % i: v[1],
                      "sr%d_at" % i: v[2]})
        for k, v in self.snap.items():
            if k == "interval_stats":
                d.update({"is_" + f: x for f, x in v.items()})
            elif k in ("max_jitter_feed", "max_jitter"):
                d["s_" + k] = bits(v)
            else:
                d["s_" + k] = v
        return d

    def sender_state(self):
        """The per-packet half, keyed as rtcp_unit --replay prints it."""
        s = self.s
        c = s.c
        return dict(initialized=1 if s.init else 0, ext_start_sn=s.start_sn, ext_highest_sn=s.high_sn,
                    ext_start_ts=s.start_ts, ext_highest_ts=s.high_ts, first_time=s.first, highest_time=s.highest_t,
                    packets_lost=c["packets_lost"], packets_padding=c["packets_padding"],
                    packets_duplicate=c["packets_duplicate"], packets_out_of_order=c["packets_out_of_order"],
                    bytes=c["bytes"], bytes_duplicate=c["bytes_duplicate"], bytes_padding=c["bytes_padding"],
                    frames=c["frames"], jitter=bits(s.jitter))


def engine_state(row):
    """An abi.SENDER_RTCP_DTYPE row as PyRtcp.state() keys it."""
    d = dict(ext_highest_sn_from_rr=int(row["ext_highest_sn_from_rr"]), last_rr_time=int(row["last_rr_time_ns"]),
             packets_lost_from_rr=int(row["packets_lost_from_rr"]), jitter_from_rr=bits(row["jitter_from_rr"]),
             max_jitter_from_rr=bits(row["max_jitter_from_rr"]), end_time=int(row["end_time_ns"]),
             last_rr_lsn=int(row["last_rr_last_sequence_number"]), last_rr_total_lost=int(row["last_rr_total_lost"]),
             rtt=int(row["rtt"]), max_rtt=int(row["max_rtt"]), nacks=int(row["nacks"]), plis=int(row["plis"]),
             firs=int(row["firs"]), clock_skew_count=int(row["clock_skew_count"]),
             out_of_order_sr_count=int(row["out_of_order_sender_report_count"]),
             cache_overflow_count=int(row["metadata_cache_overflow_count"]))
    for i, k in enumerate(("sr_first", "sr_newest")):
        sr = row[k]
        d.update({"sr%d_valid" % i: int(sr["valid"]), "sr%d_ntp" % i: int(sr["ntp"]),
                  "sr%d_rtp_ext" % i: int(sr["rtp_ext"]), "sr%d_at" % i: int(sr["at_ns"])})
    sn = row["snapshot"]
    for k in sn.dtype.names:
        if k == "interval_stats":
            d.update({"is_" + f: int(sn[k][f]) for f in IS_FIELDS})
        elif k in ("max_jitter_feed", "max_jitter"):
            d["s_" + k] = bits(sn[k])
        elif k == "start_time_ns":
            d["s_start_time"] = int(sn[k])
        else:
            d["s_" + k] = int(sn[k])
    return d


def parse_kv(line):
    """One rtcp_unit --replay output line -> (kind, {name: int}); doubles and wire bytes are hex."""
    kind, *toks = line.split()
    out = {}
    for t in toks:
        k, v = t.split("=")
        hexed = k in ("jitter", "jitter_from_rr", "max_jitter_from_rr", "s_max_jitter_feed", "s_max_jitter",
                      "jitter_max", "wire")
        out[k] = int(v, 16) if hexed and k != "wire" else (v if k == "wire" else int(v))
    return kind, out


# ---- engine + oracle + model, driven together (tests/test_rtcp_gpu.py) ------------
def _hdr_len(w):
    h = 12 + 4 * (int(w[0]) & 0xF)
    if int(w[0]) & 0x10:
        h += 4 + 4 * ((int(w[h + 2]) << 8) | int(w[h + 3]))
    return h


class Rig:
    """One trace on the oracle and (eng not None) on the engine.  The model of
    every DownTrack (PyRtcp on a PySender) is fed from the ORACLE's records:
    the forwarded packets of each batch, padding and retransmissions, in send
    order, as tests/test_sender_cpu.py replays them."""

    def __init__(self, pkg, workload, tr, eng=None):
        import ctypes as C
        import numpy as np
        from tests.oracle_lib import load as load_oracle
        self.C, self.np = C, np
        self.pkg, self.workload, self.tr, self.eng = pkg, workload, tr, eng
        self.abi = pkg.abi
        self.o = load_oracle()
        self.oh = self.o.create(500)
        workload.load_topology(self.o.api, self.oh, tr)
        if eng is not None:
            workload.load_topology(eng.api, eng.h, tr)
        self.models = [PyRtcp(PySender(int(tr.tracks[tr.downtracks[d].track].clock_rate))) for d in range(tr.ndts)]
        self.b = 0

    def close(self):
        self.o.destroy(self.oh)
        if self.eng is not None:
            self.eng.close()
        self.tr.close()

    def forward(self, nb=1, sync=True):
        """The next nb batches on both sides (the engine's only enqueued with sync=False)."""
        C, np, abi, tr = self.C, self.np, self.abi, self.tr
        for _ in range(nb):
            b = self.b
            pk, n, ar, alen = tr.batch(b)
            dd = tr.batch_dd(b)[0] if tr.has_dd() else None
            self.workload.queue_events(self.o.api, self.oh, tr, b)
            if self.eng is not None:
                self.workload.queue_events(self.eng.api, self.eng.h, tr, b)
                self.eng.submit(pk, n, ar, alen, dd)
                self.eng.run()
                if sync:
                    self.eng.sync()
            self.o.run(self.oh, pk, n, ar, alen, dd)
            rec, wire = self.pkg.drain_arrays(self.o.api, self.oh)
            pkts = np.ctypeslib.as_array(C.cast(pk, C.POINTER(C.c_uint8)), shape=(n * 64,)).view(
                np.dtype([("ext_sn", "<u8"), ("ext_ts", "<u8"), ("arrival_ns", "<i8"), ("x", "V12"),
                          ("payload_off", "<u2"), ("payload_len", "<u2"), ("y", "V24")]))
            for i in np.lexsort((np.arange(len(rec)), rec["dt"])):  # per DownTrack, send order
                r = rec[i]
                m = self.models[int(r["dt"])]
                w = wire[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])]
                p = pkts[int(r["pkt"])]
                if m.end_time == 0:
                    m.s.update(int(p["arrival_ns"]), int(r["ext_sn"]), int(r["ext_ts"]),
                               bool(r["flags"] & abi.LKF_OUT_MARKER), int(p["payload_off"]),
                               int(r["out_len"]) - _hdr_len(w), 0)
            self.b = b + 1

    def padding(self, reqs, now):
        """lkf_padding on both sides; the model takes the oracle's packets (12-B header, padding only)."""
        from tests import pad_lib
        oo, ow, _ = pad_lib.pad(self.o.api, self.oh, reqs, now)
        if self.eng is not None:
            pad_lib.pad(self.eng.api, self.eng.h, reqs, now)
        for r in oo:
            w = ow[int(r["out_off"]):int(r["out_off"]) + int(r["out_len"])]
            m = self.models[int(r["dt"])]
            if m.end_time == 0:
                m.s.update(now, int(r["ext_sn"]), int(r["ext_ts"]), bool(r["flags"] & self.abi.LKF_OUT_MARKER), 12, 0,
                           int(r["out_len"]) - _hdr_len(w))
        return len(oo)

    def rtx(self, nacks, now):
        """lkf_rtx_lookup + lkf_rtx_emit on both sides; the model takes the oracle's retransmissions."""
        from tests import rtx_lib
        idx = rtx_lib.packet_index(self.tr, self.b)
        r = rtx_lib.rtx_lookup(self.o.api, self.oh, nacks, now)
        oo, ow = rtx_lib.rtx_emit(self.o.api, self.oh, self.tr, r, idx)
        if self.eng is not None:
            g = rtx_lib.rtx_lookup(self.eng.api, self.eng.h, nacks, now)
            rtx_lib.rtx_emit(self.eng.api, self.eng.h, self.tr, g, idx)
        for q in oo:
            x = r[int(q["pkt"])]
            d = int(x["dt"])
            raw = idx[(self.tr.downtracks[d].track, int(x["layer"]), int(x["source_sn"]))]
            w = ow[int(q["out_off"]):int(q["out_off"]) + int(q["out_len"])]
            m = self.models[d]
            if m.end_time == 0:
                m.s.update(now, int(x["ext_sn"]), int(x["ext_ts"]), bool(x["marker"]), _hdr_len(raw),
                           int(q["out_len"]) - _hdr_len(w), 0)
        return len(oo)

    # -- the three calls on the engine and on the model, compared ---------------------
    def feedback(self, entries, now):
        """entries: (dt, has_rr, lsn, total_lost, jitter, lsr, dlsr, nacks, plis, firs), grouped by dt.
        -> the model's (rtt, flags) per entry, after asserting the engine's equal them."""
        np, abi = self.np, self.abi
        ent = np.zeros(len(entries), dtype=abi.RTCP_FB_DTYPE)
        want = []
        for i, (dt, has_rr, lsn, lost, jit, lsr, dlsr, nacks, plis, firs) in enumerate(entries):
            ent[i] = (dt, abi.LKF_FB_HAS_RR if has_rr else 0, lsn, lost, jit, lsr, dlsr, nacks, plis, firs, 0,
                      [0] * 7)
            m = self.models[dt]
            want.append(m.receiver_report(now, lsn, lost, jit, lsr, dlsr) if has_rr else (0, 0))
            m.counts(nacks, plis, firs)
        got = self.eng.rtcp_feedback(ent, now)
        assert [(int(g["rtt_ms"]), int(g["flags"])) for g in got] == want
        return want

    def sender_reports(self, reqs, now, ssrc_of=None):
        """reqs: (dt, calculated_clock_rate) -> the model's reports, after asserting the engine's records and
        wire bytes equal them."""
        np, abi = self.np, self.abi
        rq = np.array(reqs, dtype=abi.RTCP_SR_REQ_DTYPE)
        got, wire = self.eng.rtcp_sender_reports(rq, now, wire=True)
        want = []
        for i, (dt, ccr) in enumerate(reqs):
            m = self.models[dt]
            rep = m.sender_report(now, ccr)
            want.append(rep)
            g = got[i]
            assert int(g["dt"]) == dt
            assert {k: int(g[k]) for k in rep} == rep, (dt, rep)
            assert bytes(wire[i]) == m.sender_report_wire(rep, int(self.tr.downtracks[dt].ssrc)), dt
        return want

    def delta(self, dts):
        got = self.eng.sender_delta_info(dts)
        want = []
        for i, dt in enumerate(dts):
            d = self.models[dt].delta()
            want.append(d)
            g = got[i]
            if d is None:
                assert int(g["valid"]) == 0, dt
                continue
            e = {k: (bits(g[k]) if k == "jitter_max" else int(g[k])) for k in g.dtype.names}
            e["start_time"], e["duration"] = e.pop("start_time_ns"), e.pop("duration_ns")
            assert e == d, (dt, {k: (e.get(k), d.get(k)) for k in e if e.get(k) != d.get(k)})
        return want

    def check_state(self, dts=None):
        """The engine's whole lkf_sender_rtcp of each DownTrack against the model, and the per-packet half
        (lkf_sender_stats_get) against the PySender it stands on."""
        dts = list(range(self.tr.ndts)) if dts is None else list(dts)
        rows = self.eng.sender_rtcp(dts)
        ss = self.pkg.sender_stats(self.eng.api, self.eng.h, dts)
        for i, dt in enumerate(dts):
            m = self.models[dt]
            got, want = engine_state(rows[i]), m.state()
            assert got == want, (dt, {k: (got.get(k), want.get(k)) for k in want if got.get(k) != want.get(k)})
            s = m.sender_state()
            g = dict(initialized=int(ss[i]["initialized"]), ext_start_sn=int(ss[i]["ext_start_sn"]),
                     ext_highest_sn=int(ss[i]["ext_highest_sn"]), ext_start_ts=int(ss[i]["ext_start_ts"]),
                     ext_highest_ts=int(ss[i]["ext_highest_ts"]), first_time=int(ss[i]["first_time_ns"]),
                     highest_time=int(ss[i]["highest_time_ns"]), packets_lost=int(ss[i]["packets_lost"]),
                     packets_padding=int(ss[i]["packets_padding"]),
                     packets_duplicate=int(ss[i]["packets_duplicate"]),
                     packets_out_of_order=int(ss[i]["packets_out_of_order"]), bytes=int(ss[i]["bytes"]),
                     bytes_duplicate=int(ss[i]["bytes_duplicate"]), bytes_padding=int(ss[i]["bytes_padding"]),
                     frames=int(ss[i]["frames"]), jitter=bits(ss[i]["jitter"]))
            if s["initialized"]:
                assert g == s, (dt, {k: (g[k], s[k]) for k in s if g[k] != s[k]})
            else:
                assert g["initialized"] == 0, dt


# ---- lkf_rtcp_ingest on a Rig: the call checked against the parse's restatement (tests/rtcp_wire_lib) ----
RES_FIELDS = ("status", "fb_first", "fb_count", "reports", "nacks", "plis", "firs", "nack_first", "ref_first",
              "ref_count")
FB_FIELDS = ("flags", "last_sequence_number", "total_lost", "jitter", "last_sender_report", "delay", "nacks", "plis",
             "firs", "fraction_lost")


def ssrc(rig, dt):
    return int(rig.tr.downtracks[dt].ssrc)


def pack(pkg, entries, front=0):
    """entries (dt, bytes) -> (RTCP_RAW_DTYPE array, arena bytes, offsets).  One bytes OBJECT listed by several
    entries is laid down once: they name the same bytes.  `front` bytes of filler come first."""
    arena = bytearray(b"\xee" * front)
    raws = np.zeros(len(entries), dtype=pkg.abi.RTCP_RAW_DTYPE)
    where = {}
    for i, (dt, data) in enumerate(entries):
        if id(data) not in where:
            where[id(data)] = len(arena)
            arena += data
        raws[i] = (dt, where[id(data)], len(data))
    return raws, bytes(arena), [int(x) for x in raws["off"]]


def ingest(rig, entries, now, front=0, model=True):
    """lkf_rtcp_ingest of `entries` on rig.eng, every output compared with the restatement and (model=True)
    with the DownTracks' PyRtcp models, which advance.  -> (out, restated result dicts, NACK list)."""
    pkg = rig.pkg
    raws, arena, offs = pack(pkg, entries, front)
    res, fbs, nacks, refs, _ = W.PyRtcpIn.call(entries, lambda d: ssrc(rig, d))
    out, fb, fbo, grefs, nn = rig.eng.rtcp_ingest(raws, arena, now)
    assert len(out) == len(entries)
    for i, r in enumerate(res):
        assert {k: int(out[i][k]) for k in RES_FIELDS} == r, (i, r)
    assert len(fb) == len(fbs) == len(fbo)
    for k, (dt, f) in enumerate(fbs):
        assert int(fb[k]["dt"]) == dt and {x: int(fb[k][x]) for x in FB_FIELDS} == f, (k, f)
    assert [(int(r["entry"]), int(r["kind"]), int(r["off"]), int(r["len"])) for r in grefs] == \
        [(e, k, offs[e] + o, n) for e, k, o, n in refs]
    got = rig.eng.rtcp_ingested_nacks()
    assert nn == len(nacks) == len(got)
    assert [(int(x["dt"]), int(x["sn"])) for x in got] == nacks
    if model:
        for i, r in enumerate(res):
            rtt_report = 0
            for k in range(r["fb_first"], r["fb_first"] + r["fb_count"]):
                dt, f = fbs[k]
                m = rig.models[dt]
                want = (0, 0)
                if f["flags"] & W.FB_HAS_RR:
                    want = m.receiver_report(now, f["last_sequence_number"], f["total_lost"], f["jitter"],
                                             f["last_sender_report"], f["delay"])
                    if want[1] & FB_RTT_CHANGED:
                        rtt_report = want[0]
                m.counts(f["nacks"], f["plis"], f["firs"])
                assert (int(fbo[k]["rtt_ms"]), int(fbo[k]["flags"])) == want, (i, k)
            assert int(out[i]["rtt_ms"]) == rtt_report, i
    return out, res, nacks
