// engine.cpp — host side of liblkfwd.so (the C-ABI of include/lkfwd.h).
//
// Owns the HBM-resident per-DownTrack state and the per-batch scratch, turns
// queued control ops into a per-lane event list, and enqueues the batch
// pipeline (forward_kernels.hip).  There is no CPU forwarding path: every
// per-packet decision runs in the gfx950 kernels.
//
// Two-stage pipeline across batches.  Batch n's "decide" stage (batch init,
// track ranges, slot scan, k_decide, output scan) runs on the engine's
// high-priority decide stream after the caller's stream (which orders the
// batch's inputs); its "emit" stage (k_emit, counters) runs on a low-priority
// emit stream after an event.  The decide of batch n+1 depends only on decide
// n (DownTrack state), so it overlaps emit n.  Per-batch scratch and outputs
// live in kCtx (3) batch contexts used in turn: batch n's outputs stay valid
// until run n+kCtx is enqueued, and a device batch's input buffers must stay
// valid until its emit stage is done (lkf_sync, or the enqueue of run n+kCtx).
//
// Resources are owned by type: device buffers are DevBuf<T> (dev_buf.h),
// events, streams, graph execs and page-locked memory the owners of
// hip_own.h; deleting the engine releases them.  Every environment switch is
// a field of Knobs, read once by lkf_create.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/lkfwd.h"
#include "ctl_csr.h"
#include "dev_buf.h"
#include "fwd_state.h"
#include "handles.h"
#include "hip_own.h"
#include "kernels.h"

using namespace lkf;

namespace {

// Every device buffer the engine allocates, base -> bytes (all engines of the
// process).  Each device -> host copy of an engine buffer is checked against
// it (check_dev_range): a source range that does not lie inside one live
// allocation — a freed or reallocated buffer, or a length past the end — is
// reported as an error instead of reaching the copy engine.
struct DevRegistry {
  std::mutex m;
  std::map<uintptr_t, size_t> a;
};
DevRegistry &dreg() {
  static DevRegistry r;
  return r;
}

}  // namespace

// DevBuf's allocation functions (dev_buf.h): hipMalloc / hipFree + the registry
int lkf::dev_alloc(void **p, size_t bytes) {
  *p = nullptr;
  const hipError_t r = hipMalloc(p, bytes);
  if (r == hipSuccess) {
    std::lock_guard<std::mutex> g(dreg().m);
    dreg().a[reinterpret_cast<uintptr_t>(*p)] = bytes;
  }
  return int(r);
}

int lkf::dev_free(void *p) {
  {
    std::lock_guard<std::mutex> g(dreg().m);
    dreg().a.erase(reinterpret_cast<uintptr_t>(p));
  }
  return int(hipFree(p));
}

namespace {

// [src, src + n) inside one live allocation of this registry
bool dev_range_ok(const void *src, size_t n) {
  const uintptr_t s = reinterpret_cast<uintptr_t>(src);
  std::lock_guard<std::mutex> g(dreg().m);
  auto it = dreg().a.upper_bound(s);
  if (it == dreg().a.begin()) return false;
  --it;
  return s >= it->first && n <= it->second && s - it->first <= it->second - n;
}

constexpr int kStatsWords = 4 + LKF_DROP_NREASONS;
constexpr uint32_t kIdle = 0xffffffffu;

// Every environment switch of the engine, read once by lkf_create.  Each says
// whether it can change the results or only how the work is scheduled.
struct Knobs {
  int cuSplit = 0;              // LKF_CU_SPLIT=D: D of every 32 CUs to prep/decide, the rest to emit/sender (scheduling)
  std::string prio;             // LKF_PRIO=<decide><prep><emit><sender>, h or l each; default hhll (scheduling)
  int sideCus = 0;              // LKF_SIDE_CUS=N: the NACK side stream on the last N of every 32 CUs (scheduling)
  int emitWgPerCU = 24;         // LKF_EMIT_WG_PER_CU: the persistent emit grid's workgroups per CU (scheduling)
  bool emitPersistent = false;  // LKF_EMIT_PERSISTENT=1: emit as a persistent grid-stride launch (scheduling)
  uint32_t emitLdsPad = 5900;   // LKF_EMIT_LDS: LDS bytes reserved per emit workgroup of an ingest-fed batch (scheduling)
  uint32_t emitCapFanout = 16;  // LKF_EMIT_CAP_FANOUT: ... when it has fewer DownTracks per track than this (scheduling)
  uint32_t decideK = 0;         // LKF_DECIDE_K=0..8: DownTracks per decide wave, 0 from the batch (scheduling)
  bool hostProf = false;        // LKF_HOST_PROF=1: lkf_destroy prints lkf_run's host ms (report only)
  bool useGraph = true;         // LKF_GRAPH=0: the stages as direct launches instead of graphs (scheduling)
  bool debugDD = false;         // LKF_DEBUG_DD=1: prints the DD cursors, syncing the prep stream (scheduling)
  bool skipBktStore = false;    // LKF_SKIP_BKT_STORE=1: no bucket copies; CHANGES RESULTS (RTX from buckets goes stale)
  bool nackAlone = false;       // LKF_NACK_ALONE=1: the ingest waits for its NACK queues (scheduling)

  static Knobs from_env() {
    Knobs k;
    auto num = [](const char *name, int dflt) {
      const char *v = getenv(name);
      return v ? atoi(v) : dflt;
    };
    k.cuSplit = num("LKF_CU_SPLIT", 0);
    if (const char *v = getenv("LKF_PRIO")) k.prio = v;
    k.sideCus = num("LKF_SIDE_CUS", 0);
    k.emitWgPerCU = std::max(1, num("LKF_EMIT_WG_PER_CU", 24));
    k.emitPersistent = num("LKF_EMIT_PERSISTENT", 0) != 0;
    k.emitLdsPad = uint32_t(std::max(0, num("LKF_EMIT_LDS", 5900)));
    k.emitCapFanout = uint32_t(std::max(0, num("LKF_EMIT_CAP_FANOUT", 16)));
    k.decideK = uint32_t(std::min(8, std::max(0, num("LKF_DECIDE_K", 0))));
    k.hostProf = num("LKF_HOST_PROF", 0) != 0;
    k.useGraph = num("LKF_GRAPH", 1) != 0;
    k.debugDD = num("LKF_DEBUG_DD", 0) != 0;
    k.skipBktStore = num("LKF_SKIP_BKT_STORE", 0) != 0;
    k.nackAlone = num("LKF_NACK_ALONE", 0) != 0;
    return k;
  }
};

// A stream restricted to the CUs i with keep(i % 32) (hipExtStreamCreateWithCUMask).
template <typename Keep>
hipError_t cu_mask_stream(Stream &s, int dev, Keep keep) {
  int ncu = 256;
  (void)hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  std::vector<uint32_t> m(size_t((ncu + 31) / 32), 0);
  for (int i = 0; i < ncu; i++)
    if (keep(i % 32)) m[size_t(i / 32)] |= 1u << (i % 32);
  return hipExtStreamCreateWithCUMask(s.put(), uint32_t(m.size()), m.data());
}

// Per-batch device scratch, outputs and events (kCtx of them, used in turn).
struct BatchCtx {
  DevBuf<uint32_t> dTBegin, dTEnd, dTRuns, dErr;
  DevBuf<uint64_t> dSlotBase, dPartA, dTot;
  DevBuf<FwdRec> dRecs;    // decide -> emit: forwarded records at slotBase[dt] + j
  DevBuf<FwdBase> dFBase;  // per DownTrack: the base of its records' 32-bit SN / TS
  DevBuf<FwdBase> dWide;   // per tuple slot: a T_WIDE record's full SN / TS
  DevBuf<uint32_t> dFwdCnt;
  DevBuf<uint64_t> dFwdBytes, dRecBase, dByteBase;
  DevBuf<uint32_t> dGFirst;    // emit group g -> output position owning record 64g
  DevBuf<uint32_t> dTwccBase;  // per DownTrack: the batch's first transport-wide sequence number
  DevBuf<uint32_t> dLayerList, dLayerBefore, dLayerCnt;  // k_layer_index
  DevBuf<lkf_out> dOut;
  DevBuf<uint8_t> dOutArena;  // wire packets, or the prefixes of a prefix-mode run
  // prefix egress (allocated by the first lkf_set_egress(LKF_EGRESS_PREFIX)):
  // the records, the 64-record groups' prefix byte sums and bases, the total
  int egress = LKF_EGRESS_WIRE;  // the mode this context's run was enqueued in
  DevBuf<lkf_pre> dPre;
  DevBuf<uint32_t> dPreGSum;
  DevBuf<uint64_t> dPreGBase, dPreTot;
  DevBuf<uint64_t> dStats;
  DevBuf<lkf_pkt> dPktsOwn;  // lkf_submit copies land here
  DevBuf<uint8_t> dArenaOwn;
  DevBuf<lkf_raw_pkt> dRawPkts;  // lkf_ingest copies land here
  DevBuf<uint64_t> dBktStore;    // per datagram: what the bucket store copies (kernels.h BucketLaunch)
  // dependency descriptor (allocated with the first DD track): lkf_submit_dd
  // copies, decoded descriptors, marshalled DD bytes + their bump cursor
  DevBuf<lkf_pkt_dd> dDDIn;
  DevBuf<DDPkt> dDDPkt;
  DevBuf<uint8_t> dDDArena;
  DevBuf<uint64_t> dDDUsed;   // [0] the arena's bump cursor, [1] the spill's (u32)
  DevBuf<uint16_t> dDDSpill;  // custom frame-diff lists longer than kDDFdInline (k_dd_decode)
  DevBuf<DevEvent> dEvents;   // this batch's control ops (per-wave CSR)
  DevBuf<uint32_t> dEvOff;
  DevBuf<uint32_t> dEvLane;   // lane of each op (sorted), for k_ev_offsets
  Event prepped;   // prep stage done (prep stream)
  Event pulled;    // the control-op pull from the staging buffer done (own stream)
  Event decided;   // decide stage done (decide stream)
  Event sent;      // sender statistics done (sender stream)
  Event emitted;   // emit stage done (emit stream)
  Event ingested;  // this context's ingest done (ingest stream)
  bool fromIngest = false;        // the pending batch of this context is an ingest's output
  // that ingest also prepared the batch (k_ing_out: track ranges, zeroed
  // counters) for this topology (tracks, DownTracks); lkf_run then skips
  // k_batch_init and k_track_ranges
  bool prepByIngest = false;
  uint32_t prepNT = 0, prepND = 0;
  DevBuf<uint64_t> dITotal;    // that ingest's ExtPacket count (device; k_track_ranges reads it)
  bool used = false;
  // this context's last run had keyed ops: its resolver (k_ev_resolve, prep
  // stream) read their keys from the staging buffer, so the host rewrites the
  // staging only after that run's "prepped"
  bool keyed = false;
  // SRTP-protected copy of the output (lkf_protect; allocated on first use)
  DevBuf<uint8_t> dProt;
  bool protectedRun = false;
  // the run's descriptor (device; k_h2d pulls it from the staging buffer)
  DevBuf<RunDesc> dDesc;
  // page-locked, CPU-cached staging of the run's RunDesc + control-op CSR
  // (k_h2d reads it through the device mapping)
  StagePair stage;
  uint32_t stageCap = 0;  // ops
  // the prep stage (k_h2d ... layer index) and the decide stage's tail
  // (counters, output scan) as HIP graphs, captured for the engine's topology
  // epoch; replayed every run (one launch each instead of ~11)
  // (two prep graphs: [1] with the ingest's prep fused in — k_batch_init /
  // k_track_ranges left out — [0] without; a context alternating between an
  // ingest-prepared batch and another replays both instead of re-capturing)
  StageGraph gPrep[2], gScan, gCtl;
  // the staging or the op buffers moved: the graphs that hold their addresses
  // are re-captured by the next run (the scan tail reads neither)
  void forget_pull_graphs() { gPrep[0].epoch = gPrep[1].epoch = gCtl.epoch = 0; }
};

}  // namespace

struct lkf_engine {
  int dev = 0;
  Knobs knobs;
  // LKF_HOST_PROF=1: wall time of lkf_run's host sections (printed by lkf_destroy)
  double hp[9] = {};  // pre, stage wait, csr build, launches, total, runs, staging copies; ingest total, ingests
  CtlCsr csr;         // control-op sort (its scratch is reused from run to run)
  // The streams come first: members are destroyed in reverse order, so every
  // graph exec, event and buffer below goes before the streams do (and all of
  // them after lkf_destroy's final device sync).
  Stream own;    // copies, lookups
  Stream d2hS;   // lkf_drain_run_async's device -> host copies (created on first use)
  Stream prepS;  // ingest + batch preparation (high priority)
  // the ingests' stream (Buffer.calc): the prep stream (a non-owning view).  A
  // stream of its own (ingest n+1 beside batch n's preparation; a run's
  // preparation waits for its ingest's event, which stays) measured 9 % slower
  // on every step shape, even those without an ingest: one more high-priority
  // stream than the runtime's hardware queues, so two of the engine's streams
  // shared one (r5 A/B)
  Stream ingS;
  Stream decS;   // decide stage (high priority)
  Stream emitS;  // emit stage (low priority)
  Stream sendS;  // sender statistics of a decided batch (low priority, beside its emit)
  Stream sideS;  // an ingest's NACK queues, beside the rest of the ingest and the run
  // transport-wide sequence numbers (pion TWCC header-extension interceptor,
  // send-side BWE): a counter per transport (DownTracks bound to it count
  // together, in record order) or per unbound DownTrack
  std::vector<int32_t> dtTransport;
  DevBuf<uint32_t> dTwccCtrD, dTwccCtrT, dTwccTOff, dTwccTList;
  uint32_t nTwccT = 0;
  bool anyTwcc = false, twccDirty = false;
  Event sideFork, sideDone[2];
  bool sidePending[2] = {false, false};  // an ingest waits for the NACK queues of the one two back
  Event bktDone[2];
  bool bktPending[2] = {false, false};   // ... and for its bucket copies
  hipStream_t cur = nullptr;    // caller's stream of the last lkf_run (not owned)
  Event inEv;                   // caller-stream work before a run
  Event bktEv;                  // an ingest's bucket decisions (the sender stream copies after it)
  bool bktStorePending = false; // the next run's context waits for those copies
  lkf_cfg cfg{};
  int egress = LKF_EGRESS_WIRE;  // lkf_set_egress: the mode of the next runs
  std::string err;

  // topology (host mirror)
  std::vector<lkf_track_params> tracks;
  std::vector<uint32_t> trackDD;  // per track: DD table index or 0xffffffff
  std::vector<uint8_t> trackActive;  // 0 after lkf_remove_track
  std::vector<lkf_downtrack_params> dtp;
  std::vector<uint8_t> active;
  // the DownTrack's sequencer may hold padding exclusions (lkf_padding sent
  // packets): it is decided by k_decide_dt<true>, which carries that path
  std::vector<uint8_t> seqRM;
  bool schedDirty = true;
  std::vector<uint32_t> sched;   // lane -> dt (kIdle = padding)
  std::vector<int32_t> dtLane;   // dt -> lane (-1 inactive)
  std::vector<uint32_t> waveTrack;
  // topology added since the last flush (uploaded in one copy each)
  std::vector<DevTrack> pendTracks;
  std::vector<DTHot> pendHot;
  std::vector<DevDT> pendDTs;
  // ingress streams (host mirror + uploads pending)
  std::vector<lkf_stream_params> streams;
  std::vector<DevStream> pendStreams;
  bool spkDirty = true;

  // queued control ops
  using Pend = CtlPend;
  std::vector<Pend> pending;
  // a keyed op (lkf_at_kind other than LKF_AT_PKT) is queued: the next run
  // checks the kinds per DownTrack, stages the keys and launches the resolver
  bool keyedPending = false;
  // the pending batch is the last ingest's output (datagram keys go through
  // its scan, dPos) rather than the caller's own ExtPackets (key = index)
  bool curFromIngest = false;
  // dPos is one buffer that the next ingest overwrites: recorded after a
  // resolver that read it, waited for by the next ingest
  Event scanRead;
  bool scanReadPending = false;
  // topology epoch: bumped by every change the captured stage graphs depend
  // on (tables, schedule, DD / tracker allocations); a context re-captures
  // its graphs when its epoch is older
  uint64_t epoch = 1;
  uint64_t topoGen = 0;  // bumped by every topology change (tracks, DownTracks, streams, removals, rooms)

  // device: persistent state
  DevBuf<DevTrack> dTracks;
  DevBuf<DTHot> dHot;
  DevBuf<DTCum> dDTCum;  // per DownTrack sendingPacket totals (lkf_downtrack_summaries)
  // per DownTrack RTPStatsSender (sender_kernels.hip): statistics, gap
  // histogram, snInfo ring; host-listed updates (padding / blank / RTX)
  DevBuf<SenderStats> dSS;
  DevBuf<uint32_t> dSSGap;
  DevBuf<uint32_t> dSSRing;
  DevBuf<SenderUpd> dSSList;
  DevBuf<uint32_t> dSSGroups;  // (one more than dSSList)
  // the RTCP half of RTPStatsSender (rtcp_kernels.hip): per DownTrack state,
  // and one call's entries / groups / results (wire bytes behind the records)
  DevBuf<SenderRtcp> dRtcp;
  DevBuf<uint8_t> dRtcpIn;
  DevBuf<uint32_t> dRtcpGroups;
  DevBuf<uint8_t> dRtcpOut;
  // RTCP ingress (lkf_rtcp_ingest): one call's entries, bytes, DownTrack group
  // starts, per-entry counts / offsets / results and scan state (sized by the
  // entries), and the parsed lists (sized by the count pass's totals).  The
  // NACK list stays for lkf_rtx_lookup_ingested: riNacks sequence numbers, and
  // on the host each DownTrack's non-empty share of it (from the results).
  DevBuf<lkf_rtcp_raw> dRiIn;
  DevBuf<uint8_t> dRiArena;
  DevBuf<uint32_t> dRiGEntry, dRiFbG, dRiFbCnt, dRiRefCnt;
  DevBuf<uint64_t> dRiNackCnt, dRiFbOff, dRiNackOff, dRiRefOff, dRiTot, dRiScan;
  DevBuf<lkf_rtcp_in_result> dRiRes;
  DevBuf<lkf_rtcp_fb> dRiFb;
  DevBuf<lkf_rtcp_fb_result> dRiFbOut;
  DevBuf<lkf_nack> dRiNacks;
  DevBuf<lkf_rtcp_ref> dRiRefs;
  uint32_t riNacks = 0;
  struct RiGroup {
    int32_t dt;
    uint32_t begin, end;
  };
  std::vector<RiGroup> riGroups;
  int64_t rtxNow = 0;  // now_ns of the last lkf_rtx_lookup (the RTX packets' sendingPacket time)
  // sequencer ddBytes (sequencer.go:198-199) of the DownTracks that can forward
  // a dependency descriptor: [ring index][slot] kSeqDDBytes, grown on demand
  DevBuf<uint8_t> dSeqDD;
  DevBuf<uint32_t> dSeqDDIdx;   // per DownTrack: ring index or 0xffffffff
  DevBuf<uint32_t> dSeqDDList;  // ring index -> DownTrack; its cap() is the rings' capacity
  uint32_t nSeqDD = 0;
  std::vector<uint32_t> seqDDList;
  DevBuf<uint8_t> dRtxDD;  // lkf_rtx_emit: per record kSeqDDBytes
  // the cooperative allocation pass: per DownTrack provisional state + call buffers
  DevBuf<ProvState> dProv;
  DevBuf<lkf_prov_req> dProvReq;
  DevBuf<lkf_alloc_group> dProvGroups;
  DevBuf<uint8_t> dProvOut;  // sizeof(lkf_allocation) bytes per request
  // dependency-descriptor stream trackers (lkf_add_stream_tracker_dd)
  DevBuf<DDTrkState> dDDTrk;
  DevBuf<uint32_t> dTrackDDTrk;  // track -> DD tracker (0xffffffff none), max_tracks
  std::vector<int32_t> trackDDTrk;
  uint32_t nDDTrk = 0;
  DevBuf<int32_t> dDDTrkIds;
  DevBuf<lkf_dd_tracker_status> dDDTrkOut;
  DevBuf<DevDT> dDTs;
  DevBuf<RangeEntry> dRm;
  DevBuf<VP8Cold> dVc;
  DevBuf<SeqMeta> dSeq;
  DevBuf<uint32_t> dSched;
  DevBuf<uint32_t> dWaveTrack;  // (one more than dSched)
  DevBuf<uint32_t> dPerm;  // output position -> DownTrack (track-major)
  DevBuf<uint64_t> dCum;
  // sticky error word: every batch's decide/emit error bits (bits 0-7) and
  // every ingest's error bits (<< 8) are OR-ed in on the GPU; lkf_sync reports
  // and clears it (per-context error words are reused every kCtx runs)
  DevBuf<uint32_t> dSticky;

  // dependency-descriptor selector tables (allocated with the first DD track)
  uint32_t nDDTracks = 0;
  bool ddAlloc = false;
  DevBuf<DDStruct> dDDStruct;  // [ddIdx * kDDSlots + slot]
  DevBuf<DDTrack> dDDTrack;
  DevBuf<DDState> dDDState;    // per DownTrack
  size_t ddStateInit = 0;         // DownTracks whose DDState is zeroed
  uint32_t ddTrackInit = 0;
  std::vector<uint8_t> dtIsDD;    // per DownTrack: SVC (DD selector or VP9), scheduled in k_decide_dt<true>
  uint32_t ddLanes = 0;
  // ingress DependencyDescriptorParser per DD stream (allocated with the first)
  uint32_t nDDStreams = 0, ddStreamInit = 0;
  DevBuf<DDIngState> dDDIng;      // [stream.ddIdx]
  DevBuf<DDStruct> dDDIngStruct;  // [stream.ddIdx * 2 + DI_CUR slot]
  DevBuf<IngDD> dIngDD;           // per datagram of an ingest

  // batch input for the next run
  const lkf_pkt_dd *curDD = nullptr;
  const lkf_pkt *curPkts = nullptr;
  const uint8_t *curArena = nullptr;
  uint32_t curN = 0;
  uint64_t curArenaLen = 0;
  bool haveBatch = false;
  const uint64_t *curNDev = nullptr;  // device-side batch length (ingest-produced batch)
  bool ingestStarted = false;         // this run's start event precedes its ingest

  // three batch contexts: batch n+1 is ingested/prepared while batch n decides
  // and batch n-1 emits (its buffers are not reused until n+2)
#ifndef LKF_CTX  // batch contexts in flight (A/B)
#define LKF_CTX 3
#endif
  static constexpr int kCtx = LKF_CTX;
  BatchCtx ctx[kCtx];
  uint64_t nRuns = 0;
  int lastCtx = -1;
  // pinned bounce buffer of the host drains (D2H into caller memory that may
  // be pageable goes through it, on the engine's own stream)
  PinnedBuf bounce;

  // NACK -> RTX scratch (grown on demand; the first seven together)
  DevBuf<lkf_nack> dNacks;
  DevBuf<uint32_t> dNackG, dNackValid;  // (dNackG: one more than the rest)
  DevBuf<lkf_rtx> dRtx;
  DevBuf<lkf_raw_pkt> dRtxSrc;
  DevBuf<uint32_t> dRtxLen;
  DevBuf<uint64_t> dRtxOff;
  DevBuf<uint8_t> dRtxIn, dRtxOut;

  // stream trackers (lkf_add_stream_tracker): device state, tick scratch
  DevBuf<TrackerState> dTrk;
  uint32_t nTrk = 0;
  DevBuf<int32_t> dTrkIds;
  DevBuf<lkf_tracker_status> dTrkOut;
  // RED per-track state (lkf_red_encode / lkf_red_decode), allocated at first use
  DevBuf<RedEncState> dRedEnc;
  DevBuf<RedDecState> dRedDec;
  struct RedScratch {
    DevBuf<lkf_pkt> in, out;
    DevBuf<uint8_t> inArena, outArena;
    DevBuf<uint32_t> g, cnt;
    DevBuf<int32_t> map;
    DevBuf<uint64_t> off;
  } red;
  // lastAllocation.BandwidthRequested per DownTrack (lkf_allocate_optimal)
  DevBuf<lkf_allocation> dLastAlloc;  // lastAllocation per DownTrack
  DevBuf<lkf_alloc_req> dAllocReq;
  DevBuf<int64_t> dAllocCapacity;
  DevBuf<lkf_allocation> dAllocOut;
  // the sequencers' padding RangeMaps (SeqRM regions) and padding scratch
  DevBuf<uint8_t> dSrm;
  uint64_t srmStride = 0;
  uint32_t srmCap = 0;  // (entries of one SeqRM region, a kernel argument: not a buffer's capacity)
  DevBuf<lkf_pad_req> dPadReq;
  DevBuf<uint64_t> dPadOff;  // [2 * requests]: record bases, then arena bases
  DevBuf<uint32_t> dPadCnt;  // [2 * requests]: packets, then bytes
  DevBuf<lkf_out> dPadOut;
  DevBuf<uint8_t> dPadArena;

  // seq lookup scratch
  DevBuf<uint16_t> dSns;
  DevBuf<lkf_seq_meta> dSeqOut;
  DevBuf<uint32_t> dSeqN;

  // timing ring: [0] decide-stage start, [1] decide kernel start, [2] decide
  // kernel end (decide stream), [3] emit kernel start, [4] emit kernel end
  // (emit stream)
  static constexpr int kRing = 256;
  Event ring[kRing][5];
  uint32_t emitGrid = 2048;       // persistent grid-stride launch (LKF_EMIT_PERSISTENT=1)
  // SRTP protect (tables allocated with the first transport or lkf_protect)
  std::vector<lkf_transport_params> transports;
  DevBuf<lkf_transport_params> dTransports;
  DevBuf<SrtpKeys> dSrtpKeys;
  DevBuf<uint32_t> dAesTab;
  DevBuf<SrtpDT> dSrtpDT;
  Event protRing[256][2];        // k_srtp_roc start / k_srtp_protect end per run (timing)
  std::vector<uint8_t> protRun;  // per ring slot: that run was protected
  // SRTP unprotect (allocated with the first lkf_set_stream_transport or
  // unprotect call): per-stream receive state and its speculated copy, each
  // stream's datagram range of the call, per-datagram scratch and results
  DevBuf<SrtpRx> dSrtpRx, dSrtpRxSpec;
  DevBuf<uint32_t> dRxRange, dRxAuth;
  DevBuf<SrtpRxSpec> dRxSpec;
  DevBuf<lkf_srtp_rx_result> dRxRes;
  DevBuf<uint8_t> dSrtpStage;       // lkf_ingest_srtp's copy of the protected arena
  DevBuf<lkf_raw_pkt> dSrtpPktsIn;  // ... and of its descriptors
  Event rxRing[256][2];             // unprotect stage start / end per call (timing)
  uint64_t nUnprotects = 0;
  uint32_t lastUnprotectN = 0;
  // SRTCP: the second session key set, the receive slot tables with their
  // speculated copies and the per-call ranges (all as long as dSrtpKeys, grown
  // with it); the calls' scratch (one family per direction) and staging
  DevBuf<SrtpKeys> dSrtcpKeys;
  DevBuf<lkf_transport_srtcp> dSrtcpRx, dSrtcpRxSpec;
  DevBuf<uint32_t> dSrtcpRange;
  DevBuf<lkf_srtcp_raw> dScIn;
  DevBuf<lkf_srtcp_rx_result> dScSpec, dScRes;
  DevBuf<uint32_t> dScAuth;
  DevBuf<uint8_t> dScArena, dScPlain;  // (padded: the kernels' 16-B reads stay inside)
  DevBuf<SrtcpTx> dScTx;
  DevBuf<uint8_t> dScTxIn, dScTxOut;
  // the last lkf_srtcp_unprotect, for lkf_rtcp_ingest_unprotected: each
  // datagram's offset and plaintext length in dScPlain
  std::vector<uint32_t> scOff, scLen;
  uint64_t scPlainLen = 0;
  // ... and for lkf_rtcp_demux_unprotected each datagram's transport, and
  // whether that call's list and results reached dScIn / dScRes
  std::vector<int32_t> scTransport;
  bool scOnDevice = false;
  // RTCP demultiplexing (lkf_rtcp_demux): each DownTrack's receive-direction
  // transport; the routing table (rows by (transport, SSRC), its CSR, the rows
  // in DownTrack order, and the per-row counts / offsets / scan state, one
  // family sized by the table), rebuilt inside the next demux call when dirty;
  // one call's datagram list, bitmap rows, per-transport datagram lists,
  // results and entries
  std::vector<int32_t> dtRtcpTransport;
  bool dmxDirty = true;
  std::vector<uint32_t> dmxTFirst;  // the CSR's host copy (each transport's row count)
  uint32_t dmxRows = 0;
  DevBuf<RtcpDmxRow> dDmxRows;
  DevBuf<uint32_t> dDmxTFirst, dDmxByDt, dDmxCnt, dDmxTdFirst;
  DevBuf<uint64_t> dDmxOff, dDmxTot, dDmxScan;
  DevBuf<lkf_srtcp_raw> dDmxIn;
  DevBuf<uint32_t> dDmxBmOff, dDmxTdList, dDmxBits;
  DevBuf<uint8_t> dDmxArena;
  DevBuf<lkf_rtcp_dmx_result> dDmxRes;
  DevBuf<lkf_rtcp_entry> dDmxEntries;
  std::map<std::pair<int32_t, uint32_t>, uint32_t> scTxIndex;  // (transport, SSRC) -> the last index sent
  // ingress (one buffer.Buffer per stream) + speakers
  uint32_t maxStreams = 0;
  DevBuf<DevStream> dStreams;
  DevBuf<StreamHot> dStreamHot;
  DevBuf<uint64_t> dHist;
  DevBuf<uint32_t> dRxGap;  // per stream RTPStatsReceiver gap histogram (kGapWords u32)
  DevBuf<RangeEntry> dStreamRings;
  DevBuf<uint32_t> dTwcc;  // per datagram TWCC push word of the last ingest
  // the receivers' RTX buckets (kernels.h BucketState): per stream state, slot
  // tags / batch owners / bytes (bktSlots of dBktTag.cap() in use), per datagram slot
  DevBuf<BucketState> dBkt;
  DevBuf<uint32_t> dBktTag;
  DevBuf<uint64_t> dBktOwner;
  uint32_t bktEpoch = 0;
  DevBuf<uint8_t> dBktRing;
  uint64_t bktSlots = 0;
  DevBuf<int32_t> dBktStream;
  DevBuf<uint16_t> dBktSn;
  DevBuf<uint64_t> dPos, dIPartA, dITotal;
  DevBuf<uint32_t> dITRuns, dIErr;
  // The ingest scratch the NACK queues (side stream) and the bucket copies
  // (sender stream) read after the ingest chain has moved on: two sets,
  // alternating per ingest, so an ingest waits only for the side work of the
  // ingest two back.  ing[ingPar] is the last ingest's set.
  struct IngSet {
    DevBuf<IngParsed> parsed;
    DevBuf<lkf_flow> flows;
    DevBuf<uint32_t> fwd, tBegin, tEnd, list, listCnt;  // (list: per-stream datagram lists, k_ing_lists)
    // the ingest's RTCP NACKs: per datagram result + bump-allocated pairs
    DevBuf<uint32_t> nackInfo, nackPairOff, nackPairCnt;
    DevBuf<lkf_nack_pair> nackPairs;
    DevBuf<NackIn> nackIn;  // the NACK kernel's per-datagram input, in list order
  } ing[2];
  int ingPar = 0;
  // NACK queues (allocated with the first stream that has one)
  DevBuf<NackState> dNack;
  uint32_t nackPairCap = 0;  // (a kernel argument: the bump-allocated part of IngSet::nackPairs)
  DevBuf<uint64_t> dNackRecPos, dNackPairPos, dNackTot;
  DevBuf<uint64_t> dNackPartA;  // the compaction's scan state (side stream)
  DevBuf<lkf_rtcp_nack> dNackOut;
  DevBuf<lkf_nack_pair> dNackPairsOut;
  // ... and the same list as packets (lkf_ingest_nacks_wire), sized by its totals
  DevBuf<lkf_stream_rtcp_pkt> dNackPkts;
  DevBuf<uint8_t> dNackWire;
  // the publisher RTCP loop (rtcp_kernels.hip k_pub_*): per stream state,
  // zeroed when the stream is added, and one call's scratch family (input
  // bytes, group bounds, result bytes) with the compounds' arena beside it
  DevBuf<StreamRtcp> dStreamRtcp;
  DevBuf<uint8_t> dPubIn, dPubOut, dPubArena;
  DevBuf<uint32_t> dPubGroups;
  // Ingress frame rate (k_ing_fps; allocated with the first stream it is
  // enabled on): the enabled streams in enable order — their handles, the
  // number of the ingest that completed each (0: not yet) and their
  // calculators.  The three grow together; k_ing_fps (side stream) is the
  // only kernel that touches them.
  std::vector<int32_t> fpsHandles;
  std::vector<int32_t> fpsIdx;  // stream handle -> position in fpsHandles (-1 or beyond the end: not enabled)
  DevBuf<uint32_t> dFpsList, dFpsCalcAt;
  DevBuf<fps::State> dFps;
  uint32_t fpsEpoch = 0;  // ingests counted since the first enable
  // ... and the dependency-descriptor calculators (k_ing_fps_dd), a list of
  // their own that grows the same way; each entry has its private structure
  // pair (dFpsDDStruct[2 i], [2 i + 1]).  fpsEpoch counts for both lists.
  std::vector<int32_t> fpsDDHandles;
  std::vector<int32_t> fpsDDIdx;
  DevBuf<uint32_t> dFpsDDList, dFpsDDCalcAt;
  DevBuf<fpsdd::State> dFpsDD;
  DevBuf<DDStruct> dFpsDDStruct;
  uint32_t lastIngestN = 0;
  const lkf_raw_pkt *ingRaws = nullptr;  // the last ingest's datagram descriptors (device)
  // speaker ranking tables (rebuilt when topology changes)
  uint32_t nRooms = 0;
  DevBuf<uint32_t> dRoomPartOff, dPartId, dPartMicOff, dMics, dRoomId;
  DevBuf<lkf_speaker> dSpkSlots;
  DevBuf<uint32_t> dSpkCounts;
  std::vector<uint32_t> spkRoomIds;  // host copy of dRoomId
  // lkf_room_summaries_enqueue: the records' layout for (rows, k, s) and the
  // topology it was built for; two events order the caller's stream after the
  // packs (ingest and decide streams)
  std::vector<uint32_t> rsRooms;
  uint32_t rsK = 0, rsS = 0;
  uint64_t rsGen = ~0ull;
  DevBuf<int32_t> dRsRowEng;
  DevBuf<uint32_t> dRsSlotOff, dRsSlotDts;
  DevBuf<int64_t> dRsSlotSub;
  Event rsSpk, rsDec;
  // device -> host copies refused by the range check (CHKRANGE) since the last
  // lkf_debug_check of this engine (lkf_debug_check folds them in)
  std::atomic<uint64_t> rangeViolations{0};
  // Sender-report-driven reference-layer offsets (StreamTrackerManager,
  // streamtrackermanager.go:561-627): per track the newest sender report of
  // each layer and the offsets table as of the last queued change.  Queued
  // changes (track, at_pkt, table) expand into per-DownTrack ops of the next
  // lkf_run (kOpLayerOffsets); tracks[t].layer_offsets is the table as of the
  // last run (a DownTrack added now starts from it).
  struct TrackSR {
    uint64_t ntp[3] = {0, 0, 0};
    uint32_t rtp[3] = {0, 0, 0};
    uint8_t have[3] = {0, 0, 0};
    uint32_t offs[9] = {};
  };
  std::vector<TrackSR> trkSR;
  struct TrackOp {
    uint32_t track, at;
    uint32_t offs[9];
    int32_t kind;  // lkf_at_kind; key: the position of a keyed op
    int64_t key;
  };
  std::vector<TrackOp> trkOps;
  DevBuf<uint32_t> dDTOffs;  // per DownTrack kDTOffsWords: the offsets its Forwarder reads
  // the current batch's descriptors / DD side array are engine allocations
  // (lkf_submit / lkf_ingest*) rather than the caller's (lkf_submit_device)
  bool curOwned = false, curDDOwned = false;
};

static int fail(lkf_engine *e, const char *what, hipError_t r) {
  char buf[256];
  snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(r));
  e->err = buf;
  return LKF_EHIP;
}
#define HIPCHK(call, what)                          \
  do {                                              \
    const hipError_t _r = static_cast<hipError_t>(call);                         \
    if (_r != hipSuccess) return fail(e, what, _r); \
  } while (0)

// NewForwarder + DetermineCodec + NewRTPMunger + videolayerselector.NewBase +
// newSequencer (forwarder.go:217-338, rtpmunger.go:94, base.go NewBase,
// sequencer.go:97) as the initial HBM state of one DownTrack.
static void init_hot(DTHot &h, const lkf_track_params &tp, const lkf_downtrack_params &p) {
  std::memset(&h, 0, sizeof(h));
  h.referenceLayerSpatial = -1;
  h.maxS = h.maxT = h.seenS = h.seenT = -1;
  h.tgtS = h.tgtT = h.ptgtS = h.ptgtT = -1;
  h.curS = h.curT = h.prevS = h.prevT = -1;
  h.reqS = -1;
  h.rmOpenStart = 0;  // NewRangeMap: initRanges(0, 0)
  h.rmOpenValue = 0;
  uint32_t f = F_ACTIVE;
  if (tp.kind == LKF_KIND_VIDEO) {
    f |= F_VIDEO;
    h.maxT = 3;  // vls.SetMaxTemporal(DefaultMaxLayerTemporal) forwarder.go:235-237
    const bool svc = tp.codec == LKF_CODEC_VP9 || tp.codec == LKF_CODEC_AV1;
    if (tp.codec == LKF_CODEC_VP8) f |= F_VP8 | F_SIMULCAST | F_TLS_VP8;
    if (tp.codec == LKF_CODEC_H264) f |= F_SIMULCAST;
    if (svc && tp.has_dd) f |= F_DD;                             // DependencyDescriptor :301-334
    if (tp.codec == LKF_CODEC_VP9 && !tp.has_dd) f |= F_VP9;      // VP9 selector
    if (tp.codec == LKF_CODEC_AV1 && !tp.has_dd) f |= F_SIMULCAST;  // AV1 without DD: Simulcast
  }
  if (p.has_expected_ts) f |= F_HAS_EXPECTED;
  h.flags = f;
  h.seqStartMs = p.bind_time_ns / 1000000;
}

static bool track_has_dd(const lkf_track_params &p) {
  return p.kind == LKF_KIND_VIDEO && p.has_dd && (p.codec == LKF_CODEC_VP9 || p.codec == LKF_CODEC_AV1);
}

static DevTrack to_dev_track(const lkf_track_params &p, uint32_t ddIdx) {
  DevTrack t;
  std::memset(&t, 0, sizeof(t));
  t.ddIdx = ddIdx;
  t.kind = p.kind;
  t.codec = p.codec;
  t.hasRefTS = p.has_ref_ts;
  t.clockRate = p.clock_rate;
  for (int r = 0; r < 3; r++)
    for (int l = 0; l < 3; l++) t.layerOffsets[r * 3 + l] = p.layer_offsets[r][l];
  return t;
}

// Waits for every queued stage (run, own and emit streams).
static int drain_streams(lkf_engine *e) {
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (e->cur && e->cur != e->own) HIPCHK(hipStreamSynchronize(e->cur), "sync run stream");
  HIPCHK(hipStreamSynchronize(e->own), "sync own stream");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync ingest stream");
  HIPCHK(hipStreamSynchronize(e->prepS), "sync prep stream");
  HIPCHK(hipStreamSynchronize(e->decS), "sync decide stream");
  HIPCHK(hipStreamSynchronize(e->emitS), "sync emit stream");
  if (e->sendS) HIPCHK(hipStreamSynchronize(e->sendS), "sync sender stream");
  if (e->sideS) HIPCHK(hipStreamSynchronize(e->sideS), "sync side stream");
  return LKF_OK;
}

// A device -> host copy whose source range is not inside one live engine
// allocation (a length past a buffer's end, a freed or reallocated buffer):
// refused with LKF_EHIP and counted (lkf_debug_check folds the count into its
// violation total).  A pageable D2H copy of such a range is what surfaces as
// "an illegal memory access" from the copy call itself (the runtime's staging
// copy reads the bad range) — round 2's recorded fault was exactly that
// (a drain of tot[3] bytes past the output arena).
// every engine's refusals, for lkf_debug_check(NULL) (the whole device)
static std::atomic<uint64_t> gRangeViolationsAll{0};
static int range_fail(lkf_engine *e, const void *src, size_t n, const char *what) {
  char buf[256];
  snprintf(buf, sizeof(buf), "internal: %s: device range [%p, +%zu) outside every live engine allocation", what, src,
           n);
  e->err = buf;
  e->rangeViolations.fetch_add(1, std::memory_order_relaxed);
  gRangeViolationsAll.fetch_add(1, std::memory_order_relaxed);
  return LKF_EHIP;
}
#define CHKRANGE(src, n, what)                                                     \
  do {                                                                             \
    if ((n) && !dev_range_ok(src, n)) return range_fail(e, src, n, what);          \
  } while (0)
static int copy_to_host(lkf_engine *e, void *dst, const void *src, size_t n, const char *what);
#define D2H(dst, src, n, what)                                   \
  do {                                                           \
    const int _rc = copy_to_host(e, dst, src, n, what);          \
    if (_rc) return _rc;                                         \
  } while (0)

// Device -> caller host memory, range-checked (CHKRANGE).  A page-locked
// destination is copied directly; a pageable one (numpy arrays, std::vector,
// the stack) through the engine's pinned bounce buffer on its own stream.
static int copy_to_host(lkf_engine *e, void *dst, const void *src, size_t n, const char *what) {
  constexpr size_t kChunk = size_t(16) << 20;
  CHKRANGE(src, n, what);
  hipPointerAttribute_t pa;
  if (hipPointerGetAttributes(&pa, dst) == hipSuccess && pa.type == hipMemoryTypeHost) {  // page-locked: direct
    HIPCHK(hipMemcpy(dst, src, n, hipMemcpyDeviceToHost), what);
    return LKF_OK;
  }
  (void)hipGetLastError();  // (an unregistered pointer is not an error here)
  if (!e->bounce.p) HIPCHK(e->bounce.alloc(kChunk), "alloc bounce");
  for (size_t off = 0; off < n; off += kChunk) {
    const size_t k = std::min(kChunk, n - off);
    HIPCHK(hipMemcpyAsync(e->bounce.p, static_cast<const uint8_t *>(src) + off, k, hipMemcpyDeviceToHost, e->own), what);
    HIPCHK(hipStreamSynchronize(e->own), what);
    std::memcpy(static_cast<uint8_t *>(dst) + off, e->bounce.p, k);
  }
  return LKF_OK;
}

// hipMemcpy from pageable host memory may return before its DMA lands, and
// the engine's streams are non-blocking (they do not order against the null
// stream): every host-side upload ends with a device sync before any engine
// stream can read what it wrote.
static int upload_done(lkf_engine *e) {
  HIPCHK(hipDeviceSynchronize(), "upload sync");
  return LKF_OK;
}
static int sender_list(lkf_engine *e, std::vector<SenderUpd> &list);

// Orders the sender stream after everything queued so far on the decide, emit
// and own streams.  The per-run sender statistics run on the sender stream
// (long batches) or on the emit stream right after emit (short batches,
// k_sender_stats_thread); a control call that updates RTPStatsSender from the
// sender stream (padding, blank frames, RTX) must come after both, or a
// queued tick's Update and the call's load/store of the same SenderStats race.
static int sender_after_queued(lkf_engine *e) {
  for (hipStream_t s : {e->decS.get(), e->emitS.get(), e->own.get()}) {
    HIPCHK(hipEventRecord(e->inEv, s), "event");
    HIPCHK(hipStreamWaitEvent(e->sendS, e->inEv, 0), "wait queued stage");
  }
  return LKF_OK;
}

// The DD selector tables and per-batch DD buffers, allocated when the first
// track with the dependency-descriptor selector appears (streams drained).
static int ensure_dd(lkf_engine *e) {
  const lkf_cfg &c = e->cfg;
  if ((e->nDDTracks || e->nDDStreams) && !e->ctx[0].dDDIn)  // ingest output / lkf_submit_dd input
    for (auto &x : e->ctx) HIPCHK(x.dDDIn.alloc(c.max_batch_pkts), "alloc dd in");
  if (e->nDDStreams && !e->dDDIng) {
    HIPCHK(e->dDDIng.alloc(e->maxStreams), "alloc dd parsers");
    HIPCHK(e->dDDIngStruct.alloc(size_t(e->maxStreams) * 2), "alloc dd parser structures");
    HIPCHK(hipMemset(e->dDDIngStruct, 0, size_t(e->maxStreams) * 2 * sizeof(DDStruct)), "dd parser structures reset");
    HIPCHK(e->dIngDD.alloc(c.max_batch_pkts), "alloc ingest dd");
  }
  if (e->nDDStreams > e->ddStreamInit) {  // a fresh parser per new DD stream
    HIPCHK(hipMemset(e->dDDIng + e->ddStreamInit, 0, size_t(e->nDDStreams - e->ddStreamInit) * sizeof(DDIngState)),
           "dd parser reset");
    e->ddStreamInit = e->nDDStreams;
  }
  if (e->ddAlloc || e->nDDTracks == 0) return LKF_OK;
  HIPCHK(e->dDDStruct.alloc(size_t(c.max_tracks) * kDDSlots), "alloc dd structures");
  HIPCHK(e->dDDTrack.alloc(c.max_tracks), "alloc dd tracks");
  HIPCHK(e->dDDState.alloc(c.max_downtracks), "alloc dd state");
  HIPCHK(hipMemset(e->dDDTrack, 0, size_t(c.max_tracks) * sizeof(DDTrack)), "dd tracks reset");
  HIPCHK(hipMemset(e->dDDStruct, 0, size_t(c.max_tracks) * kDDSlots * sizeof(DDStruct)), "dd structures reset");
  const uint64_t arenaCap = c.max_out_bytes / 4 + (1u << 20);
  const uint32_t spillCap = uint32_t(std::min<uint64_t>(uint64_t(c.max_batch_pkts) * kDDFdInline + 4096, 0x7fffffffu));
  for (auto &x : e->ctx) {
    HIPCHK(x.dDDPkt.alloc(c.max_batch_pkts), "alloc dd pkts");
    HIPCHK(x.dDDArena.alloc(arenaCap), "alloc dd arena");
    HIPCHK(x.dDDUsed.alloc(2), "alloc dd cursor");
    // (zeroed here too: k_layer_index zeroes it per batch, but recycled memory
    // must never be read as a cursor; DESIGN.md §6 round-5 cursor report)
    HIPCHK(hipMemset(x.dDDUsed, 0, 2 * sizeof(uint64_t)), "dd cursor reset");
    HIPCHK(x.dDDSpill.alloc(spillCap), "alloc dd spill");
  }
  e->ddAlloc = true;
  return LKF_OK;
}

// Uploads tracks / DownTracks added since the last flush (contiguous tails).
static int flush_topology(lkf_engine *e) {
  if (e->pendTracks.empty() && e->pendDTs.empty() && e->pendStreams.empty()) return LKF_OK;
  e->epoch++;  // the stage graphs read the topology's sizes
  e->topoGen++;
  int rc = drain_streams(e);
  if (rc) return rc;
  rc = ensure_dd(e);
  if (rc) return rc;
  if (e->ddAlloc && e->ddStateInit < e->dtp.size()) {  // NewDependencyDescriptor: zero selector state
    HIPCHK(hipMemset(e->dDDState + e->ddStateInit, 0, (e->dtp.size() - e->ddStateInit) * sizeof(DDState)),
           "dd state reset");
    e->ddStateInit = e->dtp.size();
  }
  if (!e->pendTracks.empty()) {
    size_t first = e->tracks.size() - e->pendTracks.size();
    HIPCHK(hipMemcpy(e->dTracks + first, e->pendTracks.data(), e->pendTracks.size() * sizeof(DevTrack),
                     hipMemcpyHostToDevice),
           "tracks upload");
    e->pendTracks.clear();
  }
  if (!e->pendDTs.empty()) {
    size_t first = e->dtp.size() - e->pendDTs.size();
    HIPCHK(hipMemcpy(e->dHot + first, e->pendHot.data(), e->pendHot.size() * sizeof(DTHot), hipMemcpyHostToDevice),
           "hot upload");
    HIPCHK(hipMemcpy(e->dDTs + first, e->pendDTs.data(), e->pendDTs.size() * sizeof(DevDT), hipMemcpyHostToDevice),
           "dt upload");
    HIPCHK(hipMemset(e->dDTCum + first, 0, e->pendDTs.size() * sizeof(DTCum)), "dt totals reset");
    {  // the track's reference-layer offsets as of the last run (later changes arrive as ops)
      std::vector<uint32_t> ro(e->pendDTs.size() * kDTOffsWords, 0u);
      for (size_t i = 0; i < e->pendDTs.size(); i++)
        std::memcpy(&ro[i * kDTOffsWords], e->tracks[e->pendDTs[i].track].layer_offsets, 9 * sizeof(uint32_t));
      HIPCHK(hipMemcpy(e->dDTOffs + first * kDTOffsWords, ro.data(), ro.size() * sizeof(uint32_t),
                       hipMemcpyHostToDevice),
             "dt offsets upload");
    }
    {  // NewRTPStatsSender (downtrack.go:315): zero statistics at the track's clock rate
      std::vector<SenderStats> ss(e->pendDTs.size());
      std::memset(ss.data(), 0, ss.size() * sizeof(SenderStats));
      for (size_t i = 0; i < ss.size(); i++) ss[i].clockRate = e->tracks[e->pendDTs[i].track].clock_rate;
      HIPCHK(hipMemcpy(e->dSS + first, ss.data(), ss.size() * sizeof(SenderStats), hipMemcpyHostToDevice),
             "sender stats init");
      HIPCHK(hipMemset(e->dSSGap + first * kGapWords, 0, e->pendDTs.size() * kGapWords * sizeof(uint32_t)),
             "sender gap reset");
      HIPCHK(hipMemset(e->dSSRing + first * kSnInfoSize, 0, e->pendDTs.size() * kSnInfoSize * sizeof(uint32_t)),
             "sender ring reset");
      HIPCHK(hipMemset(e->dRtcp + first, 0, e->pendDTs.size() * sizeof(SenderRtcp)), "sender rtcp reset");
    }
    {  // DownTracks that can forward a DD (its selector and a negotiated extension id): a ddBytes ring
      std::vector<uint32_t> idx;
      const uint32_t n0 = e->nSeqDD;
      for (size_t i = 0; i < e->pendDTs.size(); i++) {
        const uint32_t d = uint32_t(first + i);
        const bool dd = track_has_dd(e->tracks[e->dtp[d].track]) && e->dtp[d].ext_dd != 0;
        idx.push_back(dd ? e->nSeqDD++ : 0xffffffffu);
        if (dd) e->seqDDList.push_back(d);
      }
      if (e->nSeqDD > e->dSeqDDList.cap()) {  // grow (the streams are drained): copy the rings already filled
        const uint32_t cap = std::max<uint32_t>(e->nSeqDD, 2 * uint32_t(e->dSeqDDList.cap()));
        const size_t per = size_t(e->cfg.seq_size) * kSeqDDBytes;
        // (both new buffers first: a failed allocation leaves the old rings and list as they were)
        DevBuf<uint8_t> nr;
        DevBuf<uint32_t> nl;
        HIPCHK(nr.alloc(size_t(cap) * per), "alloc sequencer dd");
        HIPCHK(nl.alloc(cap), "alloc sequencer dd list");
        HIPCHK(hipMemset(nr, 0, size_t(cap) * per), "sequencer dd reset");
        if (e->dSeqDD)
          HIPCHK(hipMemcpy(nr, e->dSeqDD, size_t(n0) * per, hipMemcpyDeviceToDevice), "sequencer dd move");
        e->dSeqDD = std::move(nr);
        e->dSeqDDList = std::move(nl);
      }
      HIPCHK(hipMemcpy(e->dSeqDDIdx + first, idx.data(), idx.size() * sizeof(uint32_t), hipMemcpyHostToDevice),
             "sequencer dd index");
      if (e->nSeqDD > n0)
        HIPCHK(hipMemcpy(e->dSeqDDList, e->seqDDList.data(), e->nSeqDD * sizeof(uint32_t), hipMemcpyHostToDevice),
               "sequencer dd list");
    }
    e->pendHot.clear();
    e->pendDTs.clear();
  }
  if (!e->pendStreams.empty()) {
    const size_t first = e->streams.size() - e->pendStreams.size();
    const size_t k = e->pendStreams.size();
    {  // RTX buckets (buffer/factory.go:31-44): audio 200 slots, video PacketBufferSize
      std::vector<BucketState> bs(k);
      uint64_t need = 0;
      for (size_t i = 0; i < k; i++) {
        const bool audio = e->tracks[e->streams[first + i].track].kind == LKF_KIND_AUDIO;
        std::memset(&bs[i], 0, sizeof(BucketState));
        bs[i].base = uint32_t(e->bktSlots + need);
        bs[i].maxSteps = audio ? 200u : e->cfg.seq_size;
        need += bs[i].maxSteps;
      }
      const uint64_t total = e->bktSlots + need;
      if (!e->dBkt) HIPCHK(e->dBkt.alloc(e->maxStreams), "alloc buckets");
      if (total > e->dBktTag.cap()) {  // grow, keeping the slots in use
        const uint64_t cap = std::max<uint64_t>(total, 2 * e->dBktTag.cap());
        DevBuf<uint32_t> tag;
        DevBuf<uint64_t> own;
        DevBuf<uint8_t> ring;
        HIPCHK(tag.alloc(cap), "alloc bucket tags");
        HIPCHK(own.alloc(cap), "alloc bucket owners");
        HIPCHK(hipMemset(own, 0, cap * sizeof(uint64_t)), "bucket owners init");  // (epochs start at 1)
        HIPCHK(ring.alloc(cap * kBktSlot), "alloc bucket ring");
        if (e->bktSlots) {
          HIPCHK(hipMemcpy(tag, e->dBktTag, e->bktSlots * 4, hipMemcpyDeviceToDevice), "bucket tags copy");
          HIPCHK(hipMemcpy(ring, e->dBktRing, e->bktSlots * kBktSlot, hipMemcpyDeviceToDevice), "bucket ring copy");
        }
        e->dBktTag = std::move(tag);
        e->dBktOwner = std::move(own);
        e->dBktRing = std::move(ring);
      }
      HIPCHK(hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(e->dBktTag + e->bktSlots), 0xFFFF0000u, need),
             "bucket tags init");  // every slot invalid (NewBucket)
      HIPCHK(hipMemcpy(e->dBkt + first, bs.data(), k * sizeof(BucketState), hipMemcpyHostToDevice), "buckets upload");
      e->bktSlots = total;
    }
    bool anyNack = false;
    for (const auto &d : e->pendStreams) anyNack = anyNack || d.nack;
    if (anyNack && !e->dNack) {  // nack.NewNACKQueue for the first Buffer with NACK feedback
      const lkf_cfg &c = e->cfg;
      HIPCHK(e->dNack.alloc(e->maxStreams), "alloc nack queues");
      HIPCHK(hipMemset(e->dNack, 0, size_t(e->maxStreams) * sizeof(NackState)), "nack queues reset");
      e->nackPairCap = uint32_t(std::min<uint64_t>(uint64_t(c.max_batch_pkts) * 8 + 4096, 1u << 30));
      // + every stream's block for the lane-parallel form (kernels.h kNackFastPairs)
      const uint64_t pairsAll = uint64_t(e->nackPairCap) + uint64_t(e->maxStreams) * kNackFastPairs;
      if (pairsAll >= (1ull << 32)) {
        e->err = "too many streams for the NACK pair buffer";
        return LKF_ENOSPC;
      }
      for (auto &g : e->ing) {
        HIPCHK(g.nackInfo.alloc(c.max_batch_pkts), "alloc nack info");
        HIPCHK(g.nackPairOff.alloc(c.max_batch_pkts), "alloc nack pair offsets");
        HIPCHK(g.nackPairCnt.alloc(1), "alloc nack pair count");
        HIPCHK(g.nackPairs.alloc(pairsAll), "alloc nack pairs");
        HIPCHK(g.nackIn.alloc(3 * size_t(c.max_batch_pkts) + 64), "alloc nack inputs");
        HIPCHK(hipMemset(g.nackInfo, 0, size_t(c.max_batch_pkts) * sizeof(uint32_t)), "nack info reset");
        HIPCHK(hipMemset(g.nackPairCnt, 0, sizeof(uint32_t)), "nack count reset");
      }
      HIPCHK(e->dNackRecPos.alloc(c.max_batch_pkts), "alloc nack positions");
      HIPCHK(e->dNackPairPos.alloc(c.max_batch_pkts), "alloc nack pair positions");
      HIPCHK(e->dNackTot.alloc(2), "alloc nack totals");
      const size_t npart = scan_state_words(c.max_batch_pkts);  // (the compaction's scan state)
      HIPCHK(e->dNackPartA.alloc(npart), "alloc nack scan state");
      HIPCHK(hipMemset(e->dNackPartA, 0, npart * sizeof(uint64_t)), "nack scan state reset");
      HIPCHK(e->dNackOut.alloc(c.max_batch_pkts), "alloc nack records");
      HIPCHK(e->dNackPairsOut.alloc(pairsAll), "alloc nack pairs out");
    }
    if (e->dNack) {  // each new queue: empty, the stream's initial RTT (0: defaultRtt)
      for (size_t i = 0; i < k; i++) {
        const uint32_t rtt = e->streams[first + i].rtt_ms ? e->streams[first + i].rtt_ms : kNackDefaultRtt;
        HIPCHK(hipMemcpy(&e->dNack[first + i].rtt, &rtt, sizeof(rtt), hipMemcpyHostToDevice), "nack rtt");
      }
    }
    std::vector<StreamHot> hot(k);
    for (auto &h : hot) {
      std::memset(&h, 0, sizeof(h));
      h.loudest = 127;  // silentAudioLevel (audiolevel.go:24)
    }
    HIPCHK(hipMemcpy(e->dStreams + first, e->pendStreams.data(), k * sizeof(DevStream), hipMemcpyHostToDevice),
           "streams upload");
    HIPCHK(hipMemcpy(e->dStreamHot + first, hot.data(), k * sizeof(StreamHot), hipMemcpyHostToDevice),
           "stream state upload");
    HIPCHK(hipMemset(e->dStreamRtcp + first, 0, k * sizeof(StreamRtcp)), "stream rtcp reset");
    HIPCHK(hipMemset(e->dHist + first * kHistWords, 0, k * kHistWords * sizeof(uint64_t)), "history reset");
    HIPCHK(hipMemset(e->dRxGap + first * kGapWords, 0, k * kGapWords * sizeof(uint32_t)), "gap histogram reset");
    e->pendStreams.clear();
  }
  return upload_done(e);
}

// Every queued stage waited for, behind the pending topology (the tracker
// calls, which no topology change reaches, pass flush = false).
static int quiesce(lkf_engine *e, bool flush = true) {
  if (flush)
    if (const int rc = flush_topology(e)) return rc;
  return drain_streams(e);
}

// One row of a per-handle table written back from the host (the engine quiesced).
template <typename T>
static int write_row(lkf_engine *e, T *dst, const T &row, const char *what) {
  HIPCHK(hipMemcpy(dst, &row, sizeof(T), hipMemcpyHostToDevice), what);
  return upload_done(e);
}

// ---- the control calls' frame ------------------------------------------------
// A control-rate call checks its handles, orders a stream, grows its scratch,
// uploads a short request list, runs one or two small kernels and hands the
// results back.  The stream and what precedes the call is one of three orders:
//   Quiesced      the engine's own stream, every stream drained first; blocking
//                 uploads, closed by uploaded() (upload_done)
//   BehindDecide  the decide stream, behind the queued decides and whatever an
//                 earlier control call left on the own stream.  The host waits
//                 for that stream alone: queued emits, sender statistics and
//                 protect stages keep overlapping the call
//   BehindSender  the sender stream, behind every queued stage that updates
//                 RTPStatsSender (sender_after_queued)
//   Ingress       the ingest stream, which owns the streams' receive state,
//                 every stream drained first as for Quiesced (the NACK queues
//                 and bucket copies of an ingest run on other streams);
//                 blocking uploads, closed by uploaded()
static int rebuild_twcc(lkf_engine *e);
enum class Order { Quiesced, BehindDecide, BehindSender, Ingress };

struct Frame {
  lkf_engine *e;
  Order order;
  hipStream_t s;
  bool grew = false;  // the last grow() reallocated its family

  Frame(lkf_engine *eng, Order o)
      : e(eng),
        order(o),
        s(o == Order::Quiesced       ? eng->own.get()
          : o == Order::BehindDecide ? eng->decS.get()
          : o == Order::Ingress      ? eng->ingS.get()
                                     : eng->sendS.get()) {}
  bool drained() const { return order == Order::Quiesced || order == Order::Ingress; }

  // flush: the pending topology first; twcc: then the transport-wide counters'
  // lists of a transport-cc DownTrack added or bound since the last run
  int open(bool flush = true, bool twcc = false) {
    if (drained()) return quiesce(e, flush);
    if (flush)
      if (const int rc = flush_topology(e)) return rc;
    HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
    if (twcc && e->twccDirty)
      if (const int rc = rebuild_twcc(e)) return rc;
    if (order == Order::BehindSender) return sender_after_queued(e);
    HIPCHK(hipEventRecord(e->inEv, e->own), "event");
    HIPCHK(hipStreamWaitEvent(s, e->inEv, 0), "wait own stream");
    return LKF_OK;
  }

  // A scratch family is freed only when nothing queued can still read it: if
  // any of its buffers is too small, the frame's stream is waited for once,
  // the whole family released, and every buffer allocated again, none smaller
  // than it was (regrow_family, dev_buf.h).  The last-listed buffer's capacity
  // is what all of them hold (the *_cap() helpers read it): after a failed
  // grow it is 0 and the next call retries.
  template <typename... T>
  int grow(const char *what, Want<T>... w) {
    grew = family_short(w...);
    if (!grew) return LKF_OK;
    HIPCHK(hipStreamSynchronize(s), "sync before a scratch family regrows");
    const int r = regrow_family(w...);
    return r ? fail(e, what, static_cast<hipError_t>(r)) : LKF_OK;
  }

  // host -> device: ahead of the frame's kernels on its stream; Quiesced and
  // Ingress: a blocking copy (uploaded() after the last one, before the first launch)
  int up(void *dst, const void *src, size_t bytes, const char *what) {
    if (drained())
      HIPCHK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), what);
    else
      HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s), what);
    return LKF_OK;
  }
  int uploaded() { return drained() ? upload_done(e) : LKF_OK; }

  // device -> host, range-checked, behind the frame's kernels: dst holds the
  // bytes after wait().  (Once the stream is idle a call may also copy with
  // D2H, through the pinned bounce buffer.)
  int down(void *dst, const void *src, size_t bytes, const char *what) {
    CHKRANGE(src, bytes, what);
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s), what);
    return LKF_OK;
  }
  int wait() {
    HIPCHK(hipStreamSynchronize(s), "sync");
    return LKF_OK;
  }
};
// a step of a frame (or any call that returns a code): return its failure
#define STEP(call)                 \
  do {                             \
    const int _rc = (call);        \
    if (_rc) return _rc;           \
  } while (0)

extern "C" {

const char *lkf_version(void) { return "lkfwd 0.2 (gfx950)"; }

const char *lkf_last_error(const lkf_engine *e) { return e ? e->err.c_str() : "null engine"; }

lkf_engine *lkf_create(int hip_device, const lkf_cfg *cfg) {
  if (!cfg) return nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || hip_device < 0 || hip_device >= ndev) return nullptr;
  if (cfg->seq_size > 65535) return nullptr;
  auto *e = new lkf_engine();
  e->dev = hip_device;
  e->cfg = *cfg;
  if (e->cfg.seq_size == 0) e->cfg.seq_size = 500;
  if (hipSetDevice(hip_device) != hipSuccess) {
    delete e;
    return nullptr;
  }
  e->knobs = Knobs::from_env();
  const Knobs &kn = e->knobs;
  const lkf_cfg &c = e->cfg;
  bool ok = true;
  auto A = [&](int r) { ok = ok && (r == int(hipSuccess)); };  // (a hipError_t, or DevBuf's int status)
  // decide is the batch-to-batch critical path: its waves should win CU slots
  // over the emit stage of the previous batch when both are resident.
  int leastPrio = 0, greatestPrio = 0;
  A(hipDeviceGetStreamPriorityRange(&leastPrio, &greatestPrio));
  A(hipStreamCreateWithFlags(e->own.put(), hipStreamNonBlocking));
  // LKF_CU_SPLIT=D (A/B): of every 32 CUs, D run the prep/decide streams and the
  // rest the emit stream (hipExtStreamCreateWithCUMask), so the latency-bound
  // decide and the HBM-bound emit of consecutive batches stop competing for
  // the same CUs; 0 (default): all CUs, decide at high priority
  if (kn.cuSplit > 0 && kn.cuSplit < 32) {
    auto low = [&](int i) { return i < kn.cuSplit; };
    auto high = [&](int i) { return i >= kn.cuSplit; };
    A(cu_mask_stream(e->decS, hip_device, low));
    A(cu_mask_stream(e->prepS, hip_device, low));
    A(cu_mask_stream(e->emitS, hip_device, high));
    A(cu_mask_stream(e->sendS, hip_device, high));
  } else {
    // LKF_PRIO=<decide><prep><emit><sender> (A/B): h(igh) or l(ow) each;
    // default "hhll" (the decide and prep chain ahead of emit for free CU slots)
    auto prio = [&](size_t i, bool hi) {
      return kn.prio.size() > i ? (kn.prio[i] == 'h' ? greatestPrio : leastPrio) : (hi ? greatestPrio : leastPrio);
    };
    A(hipStreamCreateWithPriority(e->decS.put(), hipStreamNonBlocking, prio(0, true)));
    A(hipStreamCreateWithPriority(e->prepS.put(), hipStreamNonBlocking, prio(1, true)));
    A(hipStreamCreateWithPriority(e->emitS.put(), hipStreamNonBlocking, prio(2, false)));
    A(hipStreamCreateWithPriority(e->sendS.put(), hipStreamNonBlocking, prio(3, false)));
  }
  e->ingS.view(e->prepS);
  // LKF_SIDE_CUS=N (A/B): the NACK queues' side stream on N of every 32 CUs
  // (the last N of each XCD's), so its long latency-bound waves leave the
  // other CUs to emit; 0 (default): every CU
  if (kn.sideCus > 0 && kn.sideCus < 32)
    A(cu_mask_stream(e->sideS, hip_device, [&](int i) { return i >= 32 - kn.sideCus; }));
  else
    A(hipStreamCreateWithFlags(e->sideS.put(), hipStreamNonBlocking));
  A(e->inEv.create(false));
  A(e->bktEv.create(false));
  A(e->sideFork.create(false));
  for (int i = 0; i < 2; i++) {
    A(e->sideDone[i].create(false));
    A(e->bktDone[i].create(false));
  }
  e->cur = e->own;
  A(e->dTracks.alloc(c.max_tracks));
  A(e->dHot.alloc(c.max_downtracks));
  A(e->dDTCum.alloc(c.max_downtracks));
  A(e->dTwccCtrD.alloc(c.max_downtracks));
  if (ok) A(hipMemset(e->dTwccCtrD, 0, size_t(c.max_downtracks) * sizeof(uint32_t)));
  A(e->dSS.alloc(c.max_downtracks));
  A(e->dRtcp.alloc(c.max_downtracks));
  A(e->dSeqDDIdx.alloc(c.max_downtracks));
  A(e->dSSGap.alloc(size_t(c.max_downtracks) * kGapWords));
  A(e->dSSRing.alloc(size_t(c.max_downtracks) * kSnInfoSize));
  A(e->dDTs.alloc(c.max_downtracks));
  A(e->dRm.alloc(size_t(c.max_downtracks) * kRangeCap));
  A(e->dVc.alloc(c.max_downtracks));
  A(e->dSeq.alloc(size_t(c.max_downtracks) * c.seq_size));
  e->srmCap = seqrm_cap(c.seq_size);
  e->srmStride = seqrm_stride(e->srmCap);
  A(e->dSrm.alloc(size_t(c.max_downtracks) * e->srmStride));
  A(e->dLastAlloc.alloc(c.max_downtracks));
  A(e->dCum.alloc(kStatsWords));
  A(e->dSticky.alloc(4));
  A(e->dPerm.alloc(c.max_downtracks));
  A(e->dDTOffs.alloc(size_t(c.max_downtracks) * kDTOffsWords));
  const size_t nparts = scan_state_words(c.max_downtracks);  // the slot and output scans' state
  for (auto &x : e->ctx) {
    A(x.dTBegin.alloc(c.max_tracks));
    A(x.dTEnd.alloc(c.max_tracks));
    A(x.dTRuns.alloc(c.max_tracks));
    A(x.dErr.alloc(4));
    A(x.dSlotBase.alloc(c.max_downtracks));
    A(x.dPartA.alloc(nparts));
    A(hipMemset(x.dPartA, 0, nparts * sizeof(uint64_t)));
    A(x.dTot.alloc(4));
    A(x.dRecs.alloc(c.max_batch_tuples));
    A(x.dFBase.alloc(c.max_downtracks));
    A(x.dWide.alloc(c.max_batch_tuples));
    A(x.dFwdCnt.alloc(c.max_downtracks));
    A(x.dFwdBytes.alloc(c.max_downtracks));
    A(x.dRecBase.alloc(c.max_downtracks));
    A(x.dByteBase.alloc(c.max_downtracks));
    A(x.dGFirst.alloc(c.max_out_pkts / 64 + 2));
    A(x.dTwccBase.alloc(c.max_downtracks));
    A(x.dLayerList.alloc(3 * size_t(c.max_batch_pkts) + 64));
    A(x.dLayerBefore.alloc(3 * size_t(c.max_batch_pkts) + 64));
    A(x.dLayerCnt.alloc(3 * size_t(c.max_tracks)));
    A(x.dOut.alloc(c.max_out_pkts));
    A(x.dOutArena.alloc(c.max_out_bytes + 64));
    A(x.dStats.alloc(size_t(kStatsWords) * (1 + kStatCopies)));
    A(x.dPktsOwn.alloc(c.max_batch_pkts));
    A(x.dArenaOwn.alloc(c.max_batch_arena + 64));
    A(x.dRawPkts.alloc(c.max_batch_pkts));
    A(x.dBktStore.alloc(c.max_batch_pkts));
    A(x.dDesc.alloc(1));
    A(x.dEvents.alloc(4096));
    A(x.dEvLane.alloc(4096));
    A(x.decided.create(false));
    A(x.prepped.create(false));
    A(x.pulled.create(false));
    A(x.emitted.create(false));
    A(x.ingested.create(false));
    A(x.dITotal.alloc(2));
    A(x.sent.create(false));
  }
  for (auto &r : e->ring)
    for (auto &ev : r) A(ev.create(true));
  A(e->scanRead.create(false));
  e->maxStreams = c.max_streams ? c.max_streams : 3 * c.max_tracks;
  A(e->dStreams.alloc(e->maxStreams));
  A(e->dStreamHot.alloc(e->maxStreams));
  A(e->dStreamRtcp.alloc(e->maxStreams));
  A(e->dHist.alloc(size_t(e->maxStreams) * kHistWords));
  A(e->dRxGap.alloc(size_t(e->maxStreams) * kGapWords));
  A(e->dStreamRings.alloc(size_t(e->maxStreams) * kRangeCap));
  for (auto &g : e->ing) {
    A(g.parsed.alloc(c.max_batch_pkts));
    A(g.flows.alloc(c.max_batch_pkts));
    A(g.fwd.alloc(c.max_batch_pkts));
    A(g.tBegin.alloc(c.max_tracks));
    A(g.tEnd.alloc(c.max_tracks));
    A(g.list.alloc(3 * size_t(c.max_batch_pkts) + 64));
    A(g.listCnt.alloc(3 * size_t(c.max_tracks)));
  }
  A(e->dTwcc.alloc(c.max_batch_pkts));
  A(e->dPos.alloc(c.max_batch_pkts));
  const size_t ipart = scan_state_words(c.max_batch_pkts);  // the ingest scan's state
  A(e->dIPartA.alloc(ipart));
  A(hipMemset(e->dIPartA, 0, ipart * sizeof(uint64_t)));
  A(e->dITotal.alloc(2));
  A(e->dITRuns.alloc(c.max_tracks));
  A(e->dIErr.alloc(4));
  if (ok) {
    A(hipMemset(e->dSeq, 0, size_t(c.max_downtracks) * c.seq_size * sizeof(SeqMeta)));
    // Every persistent table starts zeroed: hipMalloc hands back memory an
    // earlier engine of the process wrote, and no kernel may ever see those
    // bytes (the rings are read only below their counts, but a zero start
    // makes every batch's inputs the same from one process to the next).
    A(hipMemset(e->dRm, 0, size_t(c.max_downtracks) * kRangeCap * sizeof(RangeEntry)));
    A(hipMemset(e->dVc, 0, size_t(c.max_downtracks) * sizeof(VP8Cold)));
    A(hipMemset(e->dSrm, 0, size_t(c.max_downtracks) * e->srmStride));
    A(hipMemset(e->dHot, 0, size_t(c.max_downtracks) * sizeof(DTHot)));
    A(hipMemset(e->dDTs, 0, size_t(c.max_downtracks) * sizeof(DevDT)));
    A(hipMemset(e->dDTCum, 0, size_t(c.max_downtracks) * sizeof(DTCum)));
    A(hipMemset(e->dSeqDDIdx, 0xff, size_t(c.max_downtracks) * sizeof(uint32_t)));
    A(hipMemset(e->dTracks, 0, size_t(c.max_tracks) * sizeof(DevTrack)));
    A(hipMemset(e->dStreamHot, 0, size_t(e->maxStreams) * sizeof(StreamHot)));
    A(hipMemset(e->dStreamRtcp, 0, size_t(e->maxStreams) * sizeof(StreamRtcp)));
    A(hipMemset(e->dStreamRings, 0, size_t(e->maxStreams) * kRangeCap * sizeof(RangeEntry)));
    A(hipMemset(e->dHist, 0, size_t(e->maxStreams) * kHistWords * sizeof(uint64_t)));
    {  // VideoAllocationDefault (forwarder.go:111-116)
      lkf_allocation d = {};
      d.pause_reason = 3;
      d.target_spatial = d.target_temporal = d.request_spatial = d.max_spatial = d.max_temporal = -1;
      std::vector<lkf_allocation> v(c.max_downtracks, d);
      A(hipMemcpy(e->dLastAlloc, v.data(), v.size() * sizeof(lkf_allocation), hipMemcpyHostToDevice));
    }
    A(hipMemset(e->dCum, 0, kStatsWords * sizeof(uint64_t)));
    A(hipMemset(e->dSticky, 0, 4 * sizeof(uint32_t)));
    for (auto &x : e->ctx) {
      A(hipMemset(x.dArenaOwn, 0, c.max_batch_arena + 64));
      A(hipMemset(x.dTot, 0, 4 * sizeof(uint64_t)));
      A(hipMemset(x.dStats, 0, size_t(kStatsWords) * (1 + kStatCopies) * sizeof(uint64_t)));
      A(hipMemset(x.dErr, 0, 4 * sizeof(uint32_t)));
    }
    // hipMemset runs on the null stream, which the engine's non-blocking
    // streams do not wait for: finish the initialisation before any batch
    // (a late zero-fill raced the first batch's arena copy and sequencer writes)
    A(hipDeviceSynchronize());
  }
  if (!ok) {
    lkf_destroy(e);
    return nullptr;
  }
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, hip_device);
  // emit is grid-stride with one-wave workgroups: 24 waves per CU saturate
  // HBM and leave wave slots for the next batch's decide stage.
  e->emitGrid = uint32_t(cus) * uint32_t(kn.emitWgPerCU);
  return e;
}

void lkf_destroy(lkf_engine *e) {
  if (!e) return;
  if (e->knobs.hostProf && e->hp[5] > 0)
    fprintf(stderr,
            "lkf host ms/run: pre %.4f stage-wait %.4f csr %.4f copies %.4f launches %.4f total %.4f (%d runs)\n",
            e->hp[0] / e->hp[5], e->hp[1] / e->hp[5], e->hp[2] / e->hp[5], e->hp[6] / e->hp[5],
            e->hp[3] / e->hp[5], e->hp[4] / e->hp[5], int(e->hp[5]));
  if (e->knobs.hostProf && e->hp[8] > 0)
    fprintf(stderr, "lkf host ms/ingest: %.4f (%d ingests: the launches of the Buffer.calc chain, no host wait)\n",
            e->hp[7] / e->hp[8], int(e->hp[8]));
  (void)hipSetDevice(e->dev);
  if (e->cur && e->cur != e->own) (void)hipStreamSynchronize(e->cur);
  if (e->own) (void)hipStreamSynchronize(e->own);
  if (e->ingS) (void)hipStreamSynchronize(e->ingS);
  if (e->prepS) (void)hipStreamSynchronize(e->prepS);
  if (e->decS) (void)hipStreamSynchronize(e->decS);
  if (e->emitS) (void)hipStreamSynchronize(e->emitS);
  if (e->sendS) (void)hipStreamSynchronize(e->sendS);  // (bucket copies, sender updates)
  if (e->sideS) (void)hipStreamSynchronize(e->sideS);  // (NACK queues)
  if (e->d2hS) (void)hipStreamSynchronize(e->d2hS);    // (asynchronous drains)
  (void)hipDeviceSynchronize();                        // (anything else queued before the buffers go)
  delete e;  // the members release every buffer, event, graph exec and stream (streams last)
}

int32_t lkf_add_track(lkf_engine *e, const lkf_track_params *p) {
  if (!e || !p) return LKF_EINVAL;
  if (e->tracks.size() >= e->cfg.max_tracks) return LKF_ENOSPC;
  int32_t h = int32_t(e->tracks.size());
  e->tracks.push_back(*p);
  uint32_t ddIdx = 0xffffffffu;
  if (track_has_dd(*p)) ddIdx = e->nDDTracks++;
  e->trackDD.push_back(ddIdx);
  e->trackActive.push_back(1);
  e->trkSR.emplace_back();
  std::memcpy(e->trkSR.back().offs, p->layer_offsets, 9 * sizeof(uint32_t));
  e->pendTracks.push_back(to_dev_track(*p, ddIdx));  // uploaded by flush_topology
  e->schedDirty = true;
  return h;
}

// an op's position: (LKF_AT_PKT, at_pkt) or a key of another kind
static bool at_key_valid(int32_t kind, int64_t key) {
  if (kind == LKF_AT_PKT) return key >= 0 && key <= int64_t(0xffffffffu);
  if (kind == LKF_AT_DATAGRAM) return key >= 0;
  return kind == LKF_AT_ARRIVAL_NS;
}

int lkf_set_layer_offsets_key(lkf_engine *e, int32_t track, const uint32_t offsets[9], int32_t kind, int64_t key) {
  if (!e || !offsets || track < 0 || track >= int32_t(e->tracks.size())) return LKF_EINVAL;
  if (!at_key_valid(kind, key)) return LKF_EINVAL;
  lkf_engine::TrackOp op;
  op.track = uint32_t(track);
  op.at = kind == LKF_AT_PKT ? uint32_t(key) : 0u;
  op.kind = kind;
  op.key = key;
  std::memcpy(op.offs, offsets, sizeof(op.offs));
  std::memcpy(e->trkSR[size_t(track)].offs, offsets, sizeof(op.offs));
  e->trkOps.push_back(op);
  if (kind != LKF_AT_PKT) e->keyedPending = true;
  return LKF_OK;
}

int lkf_set_layer_offsets_at(lkf_engine *e, int32_t track, const uint32_t offsets[9], uint32_t at_pkt) {
  return lkf_set_layer_offsets_key(e, track, offsets, LKF_AT_PKT, int64_t(at_pkt));
}

int lkf_set_layer_offsets(lkf_engine *e, int32_t track, const uint32_t offsets[9]) {
  return lkf_set_layer_offsets_at(e, track, offsets, 0);
}

// mediatransportutil v0.0.0-20231213075826-cccbf2b93d3f NtpTime.Duration (the
// offset of NtpTime.Time from the NTP epoch): seconds, and the 32-bit fraction
// in nanoseconds rounded half up
static int64_t ntp_ns(uint64_t t) {
  const uint64_t sec = (t >> 32) * 1000000000ull;
  const uint64_t frac = (t & 0xffffffffull) * 1000000000ull;
  uint64_t nsec = frac >> 32;
  if (uint32_t(frac) >= 0x80000000u) nsec++;
  return int64_t(sec + nsec);
}

// StreamTrackerManager.updateLayerOffsetLocked (streamtrackermanager.go:561-601)
static bool sr_layer_offset(lkf_engine::TrackSR &s, uint32_t clockRate, int ref, int other) {
  if (!s.have[ref] || s.ntp[ref] == 0 || !s.have[other] || s.ntp[other] == 0) return false;
  const int64_t d = ntp_ns(s.ntp[ref]) - ntp_ns(s.ntp[other]);  // srRef.Time().Sub(srOther.Time())
  const double secs = double(d / 1000000000) + double(d % 1000000000) / 1e9;  // Duration.Seconds
  if (std::fabs(secs) > 60.0) return false;  // senderReportThresholdSeconds :36
  const int64_t rtpDiff = d * int64_t(clockRate) / 1000000000;
  const uint32_t norm = s.rtp[other] + uint32_t(rtpDiff);
  uint32_t off = s.rtp[ref] - norm;
  if (off == 0) off = 1;
  const bool changed = s.offs[ref * 3 + other] != off;
  s.offs[ref * 3 + other] = off;
  return changed;
}

// SetRTCPSenderReportData (streamtrackermanager.go:603-627)
int lkf_sender_report_key(lkf_engine *e, int32_t track, int32_t layer, uint64_t ntp_timestamp, uint32_t rtp_timestamp,
                          int32_t kind, int64_t key) {
  if (!e || track < 0 || track >= int32_t(e->tracks.size())) return LKF_EINVAL;
  if (!at_key_valid(kind, key)) return LKF_EINVAL;
  if (layer < 0 || layer > 2) return LKF_OK;  // (invalid layer: ignored, as the reference)
  lkf_engine::TrackSR &s = e->trkSR[size_t(track)];
  s.ntp[layer] = ntp_timestamp;
  s.rtp[layer] = rtp_timestamp;
  s.have[layer] = 1;
  bool changed = false;
  for (int i = 0; i < 3; i++) {
    if (i == layer) continue;
    changed |= sr_layer_offset(s, e->tracks[size_t(track)].clock_rate, layer, i);
    changed |= sr_layer_offset(s, e->tracks[size_t(track)].clock_rate, i, layer);
  }
  if (!changed) return LKF_OK;
  lkf_engine::TrackOp op;
  op.track = uint32_t(track);
  op.at = kind == LKF_AT_PKT ? uint32_t(key) : 0u;
  op.kind = kind;
  op.key = key;
  std::memcpy(op.offs, s.offs, sizeof(op.offs));
  e->trkOps.push_back(op);
  if (kind != LKF_AT_PKT) e->keyedPending = true;
  return LKF_OK;
}

int lkf_sender_report(lkf_engine *e, int32_t track, int32_t layer, uint64_t ntp_timestamp, uint32_t rtp_timestamp,
                      uint32_t at_pkt) {
  return lkf_sender_report_key(e, track, layer, ntp_timestamp, rtp_timestamp, LKF_AT_PKT, int64_t(at_pkt));
}

int32_t lkf_add_downtrack(lkf_engine *e, const lkf_downtrack_params *p) {
  if (!e || !p) return LKF_EINVAL;
  if (p->track < 0 || p->track >= int32_t(e->tracks.size())) return LKF_EINVAL;
  if (e->dtp.size() >= e->cfg.max_downtracks) return LKF_ENOSPC;
  int32_t h = int32_t(e->dtp.size());
  e->dtp.push_back(*p);
  e->active.push_back(1);
  e->seqRM.push_back(0);
  {  // DD selector and VP9 SVC DownTracks: k_decide_dt<true> (svc_run)
    const lkf_track_params &tp = e->tracks[p->track];
    const bool vp9 = tp.kind == LKF_KIND_VIDEO && tp.codec == LKF_CODEC_VP9;
    e->dtIsDD.push_back((track_has_dd(tp) || vp9) ? 1 : 0);
  }
  e->pendHot.emplace_back();
  init_hot(e->pendHot.back(), e->tracks[p->track], *p);
  DevDT d;
  std::memset(&d, 0, sizeof(d));
  d.track = uint32_t(p->track);
  d.ssrc = p->ssrc;
  d.pt = p->payload_type;
  d.extPlayout = p->ext_playout;
  d.extAbs = p->ext_abs_send_time;
  d.extDD = p->ext_dd;
  d.extTcc = p->ext_transport_cc;
  d.twccGroup = uint32_t(h);  // its own counter until bound to a transport
  std::memcpy(d.playout, p->playout_delay, 3);
  d.active = 1;
  e->dtTransport.push_back(-1);
  e->dtRtcpTransport.push_back(-1);
  e->dmxDirty = true;
  if (p->ext_transport_cc) e->anyTwcc = e->twccDirty = true;
  e->pendDTs.push_back(d);  // uploaded by flush_topology (one copy per batch of adds)
  e->schedDirty = true;
  return h;
}

// rtpStatsBase.Stop (DownTrack.CloseWithFlush): endTime set, a mark (streams drained)
static int rtcp_stop(lkf_engine *e, size_t dt) {
  const int64_t mark = 1;
  HIPCHK(hipMemcpy(reinterpret_cast<uint8_t *>(e->dRtcp + dt) + offsetof(SenderRtcp, endTime), &mark, sizeof(mark),
                   hipMemcpyHostToDevice),
         "rtcp stop copy");
  return LKF_OK;
}

int lkf_remove_downtrack(lkf_engine *e, int32_t dt) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  e->active[dt] = 0;
  e->dmxDirty = true;
  e->topoGen++;
  uint8_t zero = 0;
  HIPCHK(hipMemcpy(reinterpret_cast<uint8_t *>(e->dDTs + dt) + offsetof(DevDT, active), &zero, 1,
                   hipMemcpyHostToDevice),
         "remove copy");
  STEP(rtcp_stop(e, size_t(dt)));
  e->schedDirty = true;
  return upload_done(e);
}

int lkf_remove_track(lkf_engine *e, int32_t track) {
  if (!e || track < 0 || track >= int32_t(e->tracks.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  if (!e->trackActive[track]) return LKF_OK;
  e->trackActive[track] = 0;
  const uint8_t zero = 0, one = 1;
  for (size_t d = 0; d < e->dtp.size(); d++)  // closeTracks: every DownTrack of the receiver
    if (e->dtp[d].track == track && e->active[d]) {
      e->active[d] = 0;
      e->dmxDirty = true;
      e->topoGen++;
      HIPCHK(hipMemcpy(reinterpret_cast<uint8_t *>(e->dDTs + d) + offsetof(DevDT, active), &zero, 1,
                       hipMemcpyHostToDevice),
             "remove copy");
      STEP(rtcp_stop(e, d));
    }
  for (size_t sid = 0; sid < e->streams.size(); sid++)  // Buffer.Close of its streams
    if (e->streams[sid].track == track)
      HIPCHK(hipMemcpy(reinterpret_cast<uint8_t *>(e->dStreams + sid) + offsetof(DevStream, closed), &one, 1,
                       hipMemcpyHostToDevice),
             "close copy");
  e->schedDirty = true;
  e->spkDirty = true;
  return upload_done(e);
}

static_assert(sizeof(lkf_ctl_event_key) == 56, "lkf_ctl_event_key is 56 B");

int lkf_ctl_key(lkf_engine *e, int32_t dt, int32_t op, int64_t a0, int64_t a1, int64_t a2, int64_t a3, int32_t kind,
                int64_t key) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  if (op < LKF_CTL_MUTE || op > LKF_CTL_PLAYOUT_ACKED) return LKF_EINVAL;
  if (!at_key_valid(kind, key)) return LKF_EINVAL;
  lkf_engine::Pend p;
  p.dt = uint32_t(dt);
  std::memset(&p.ev, 0, sizeof(p.ev));
  p.ev.at = kind == LKF_AT_PKT ? uint32_t(key) : 0u;
  p.ev.op = op;
  p.ev.a[0] = a0;
  p.ev.a[1] = a1;
  p.ev.a[2] = a2;
  p.ev.a[3] = a3;
  p.key = key;
  p.kind = kind;
  e->pending.push_back(p);
  if (kind != LKF_AT_PKT) e->keyedPending = true;
  return LKF_OK;
}

int lkf_ctl_batch_key(lkf_engine *e, const lkf_ctl_event_key *evs, uint32_t n) {
  if (!e || (n && !evs)) return LKF_EINVAL;
  const int32_t nd = int32_t(e->dtp.size());
  for (uint32_t i = 0; i < n; i++)
    if (evs[i].dt < 0 || evs[i].dt >= nd || evs[i].op < LKF_CTL_MUTE || evs[i].op > LKF_CTL_PLAYOUT_ACKED ||
        !at_key_valid(evs[i].kind, evs[i].key))
      return LKF_EINVAL;
  e->pending.reserve(e->pending.size() + n);
  for (uint32_t i = 0; i < n; i++) {
    lkf_engine::Pend p;
    p.dt = uint32_t(evs[i].dt);
    std::memset(&p.ev, 0, sizeof(p.ev));
    p.ev.at = evs[i].kind == LKF_AT_PKT ? uint32_t(evs[i].key) : 0u;
    p.ev.op = evs[i].op;
    for (int j = 0; j < 4; j++) p.ev.a[j] = evs[i].a[j];
    p.key = evs[i].key;
    p.kind = evs[i].kind;
    e->pending.push_back(p);
    if (p.kind != LKF_AT_PKT) e->keyedPending = true;
  }
  return LKF_OK;
}

int lkf_ctl(lkf_engine *e, int32_t dt, int32_t op, int64_t a0, int64_t a1, int64_t a2, int64_t a3, uint32_t at_pkt) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  if (op < LKF_CTL_MUTE || op > LKF_CTL_PLAYOUT_ACKED) return LKF_EINVAL;
  lkf_engine::Pend p;
  p.dt = uint32_t(dt);
  std::memset(&p.ev, 0, sizeof(p.ev));
  p.key = 0;
  p.kind = LKF_AT_PKT;
  p.ev.at = at_pkt;
  p.ev.op = op;
  p.ev.a[0] = a0;
  p.ev.a[1] = a1;
  p.ev.a[2] = a2;
  p.ev.a[3] = a3;
  e->pending.push_back(p);
  return LKF_OK;
}

int lkf_ctl_batch(lkf_engine *e, const lkf_ctl_event *evs, uint32_t n) {
  if (!e || (n && !evs)) return LKF_EINVAL;
  const int32_t nd = int32_t(e->dtp.size());
  for (uint32_t i = 0; i < n; i++)
    if (evs[i].dt < 0 || evs[i].dt >= nd || evs[i].op < LKF_CTL_MUTE || evs[i].op > LKF_CTL_PLAYOUT_ACKED)
      return LKF_EINVAL;
  e->pending.reserve(e->pending.size() + n);
  for (uint32_t i = 0; i < n; i++) {
    lkf_engine::Pend p;
    p.dt = uint32_t(evs[i].dt);
    std::memset(&p.ev, 0, sizeof(p.ev));
    p.key = 0;
    p.kind = LKF_AT_PKT;
    p.ev.at = evs[i].at_pkt;
    p.ev.op = evs[i].op;
    for (int j = 0; j < 4; j++) p.ev.a[j] = evs[i].a[j];
    e->pending.push_back(p);
  }
  return LKF_OK;
}

int lkf_submit(lkf_engine *e, const lkf_pkt *pkts, uint32_t n, const uint8_t *arena, uint64_t arena_len) {
  if (!e || (n && !pkts)) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts || arena_len > e->cfg.max_batch_arena) return LKF_ENOSPC;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[e->nRuns % lkf_engine::kCtx];
  if (x.used) HIPCHK(hipEventSynchronize(x.emitted), "wait emit");  // batch n-2 still reads these buffers
  if (n) HIPCHK(hipMemcpyAsync(x.dPktsOwn, pkts, size_t(n) * sizeof(lkf_pkt), hipMemcpyHostToDevice, e->own), "pkts");
  if (arena_len) HIPCHK(hipMemcpyAsync(x.dArenaOwn, arena, arena_len, hipMemcpyHostToDevice, e->own), "arena");
  HIPCHK(hipStreamSynchronize(e->own), "submit sync");
  x.prepByIngest = false;
  e->curPkts = x.dPktsOwn;
  e->curArena = x.dArenaOwn;
  e->curN = n;
  e->curNDev = nullptr;
  e->curDD = nullptr;
  e->curOwned = true;
  e->curDDOwned = true;
  e->curFromIngest = false;
  e->ingestStarted = false;
  e->curArenaLen = arena_len;
  e->haveBatch = true;
  return LKF_OK;
}

int lkf_submit_device(lkf_engine *e, const lkf_pkt *d_pkts, uint32_t n, const uint8_t *d_arena, uint64_t arena_len) {
  if (!e || (n && !d_pkts)) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts) return LKF_ENOSPC;
  e->ctx[e->nRuns % lkf_engine::kCtx].prepByIngest = false;
  e->curPkts = d_pkts;
  e->curArena = d_arena;
  e->curN = n;
  e->curNDev = nullptr;
  e->curDD = nullptr;
  e->curOwned = false;
  e->curDDOwned = true;
  e->curFromIngest = false;
  e->ingestStarted = false;
  e->curArenaLen = arena_len;
  e->haveBatch = true;
  return LKF_OK;
}

int lkf_submit_dd(lkf_engine *e, const lkf_pkt_dd *dd, uint32_t n) {
  if (!e || (n && !dd)) return LKF_EINVAL;
  if (!e->haveBatch || n != e->curN) return LKF_EINVAL;  // parallel to the batch just submitted
  int rc = flush_topology(e);
  if (rc) return rc;
  if (!e->ddAlloc) return LKF_OK;  // no DD track: nothing reads it
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[e->nRuns % lkf_engine::kCtx];
  if (x.used) HIPCHK(hipEventSynchronize(x.emitted), "wait emit");  // batch n-3 may still read it
  if (n) HIPCHK(hipMemcpyAsync(x.dDDIn, dd, size_t(n) * sizeof(lkf_pkt_dd), hipMemcpyHostToDevice, e->own), "dd");
  HIPCHK(hipStreamSynchronize(e->own), "submit dd sync");
  e->curDD = x.dDDIn;
  e->curDDOwned = true;
  return LKF_OK;
}

int lkf_submit_dd_device(lkf_engine *e, const lkf_pkt_dd *d_dd, uint32_t n) {
  if (!e || (n && !d_dd)) return LKF_EINVAL;
  if (!e->haveBatch || n != e->curN) return LKF_EINVAL;
  e->curDD = d_dd;
  e->curDDOwned = false;
  return LKF_OK;
}

// Lane schedule: one wave per (track, up to 64 of its DownTracks), idle lanes
// padded with kIdle.  Video tracks first (longest packet lists).
static int rebuild_sched(lkf_engine *e) {
  const uint32_t nd = uint32_t(e->dtp.size());
  const uint32_t nt = uint32_t(e->tracks.size());
  std::vector<std::vector<uint32_t>> byTrack(nt);
  for (uint32_t d = 0; d < nd; d++)
    if (e->active[d]) byTrack[e->dtp[d].track].push_back(d);
  std::vector<uint32_t> order(nt);
  for (uint32_t t = 0; t < nt; t++) order[t] = t;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return e->tracks[a].kind > e->tracks[b].kind; });
  // Two parts: DownTracks of the plain selectors (k_decide_dt<false>), then
  // the SVC ones (dependency-descriptor or VP9 selector) and those whose
  // sequencer holds padding exclusions (k_decide_dt<true>), each interleaved
  // per XCD.
  std::vector<uint32_t> sched, waveTrack;
  e->ddLanes = 0;
  for (int part = 0; part < 2; part++) {
    std::vector<uint32_t> ps, pt;
    for (uint32_t t : order) {
      for (uint32_t d : byTrack[t]) {  // one wave per DownTrack (interleaved per XCD below)
        if ((e->dtIsDD[d] || e->seqRM[d]) != (part == 1)) continue;
        ps.push_back(d);
        pt.push_back(t);
      }
    }
    if (ps.empty()) continue;
    // Waves are dispatched round-robin over the 8 XCDs (block b -> XCD b % 8).
    // Give all DownTracks of a track the same XCD, consecutive in its order,
    // so the 8-9 waves reading one track's packet descriptors share an L2.
    // Tracks go to the XCD with the fewest waves so far (video first, so the
    // long waves spread evenly); idle slots pad the shorter XCD lists.
    constexpr int kX = 8;
    std::vector<std::vector<uint32_t>> lst(kX), lstT(kX);
    std::vector<double> load(kX, 0.0);
    size_t i = 0;
    while (i < ps.size()) {
      const uint32_t t = pt[i];
      size_t j = i;
      while (j < ps.size() && pt[j] == t) j++;
      int bx = 0;
      for (int x = 1; x < kX; x++)
        if (load[x] < load[bx]) bx = x;
      const double w = e->tracks[t].kind == LKF_KIND_VIDEO ? 7.0 : 1.0;  // ~packets per wave
      for (size_t q = i; q < j; q++) {
        lst[bx].push_back(ps[q]);
        lstT[bx].push_back(t);
        load[bx] += w;
      }
      i = j;
    }
    size_t mx = 0;
    for (auto &l : lst) mx = std::max(mx, l.size());
    const size_t base = sched.size();
    sched.resize(base + mx * kX, kIdle);
    waveTrack.resize(base + mx * kX, 0);
    for (int x = 0; x < kX; x++)
      for (size_t q = 0; q < lst[x].size(); q++) {
        sched[base + q * kX + x] = lst[x][q];
        waveTrack[base + q * kX + x] = lstT[x][q];
      }
    if (part == 1) e->ddLanes = uint32_t(mx * kX);
  }
  e->sched.swap(sched);
  e->waveTrack.swap(waveTrack);
  e->dtLane.assign(nd, -1);
  for (uint32_t l = 0; l < e->sched.size(); l++)
    if (e->sched[l] != kIdle) e->dtLane[e->sched[l]] = int32_t(l);
  const size_t nl = e->sched.size();
  int rc = drain_streams(e);  // queued runs still read the previous schedule
  if (rc) return rc;
  if (nl + 1 > e->dSched.cap() || nl + 2 > e->dWaveTrack.cap()) {
    release_all(e->dSched, e->dWaveTrack);
    HIPCHK(e->dSched.alloc(nl + 1 + 4096), "alloc sched");
    HIPCHK(e->dWaveTrack.alloc(nl + 2 + 4096), "alloc wavetrack");
  }
  // output order: by track, then DownTrack handle (every DownTrack, active or not)
  {
    std::vector<uint32_t> perm(nd);
    for (uint32_t d = 0; d < nd; d++) perm[d] = d;
    std::stable_sort(perm.begin(), perm.end(),
                     [&](uint32_t a, uint32_t b) { return e->dtp[a].track < e->dtp[b].track; });
    if (nd) HIPCHK(hipMemcpy(e->dPerm, perm.data(), nd * sizeof(uint32_t), hipMemcpyHostToDevice), "perm copy");
  }
  if (nl) {
    HIPCHK(hipMemcpy(e->dSched, e->sched.data(), nl * sizeof(uint32_t), hipMemcpyHostToDevice), "sched copy");
    HIPCHK(hipMemcpy(e->dWaveTrack, e->waveTrack.data(), e->waveTrack.size() * sizeof(uint32_t),
                     hipMemcpyHostToDevice),
           "wavetrack copy");
  }
  e->schedDirty = false;
  e->epoch++;
  return upload_done(e);
}

// Per transport, its transport-cc DownTracks in record order (track, then
// DownTrack handle) for k_twcc_base; the counters of transports added since
// the last rebuild start at 0 (pion's interceptor starts at 0 per
// PeerConnection).  Queued runs read the lists: drained first.
static int rebuild_twcc(lkf_engine *e) {
  int rc = drain_streams(e);
  if (rc) return rc;
  const uint32_t nt = uint32_t(e->transports.size());
  std::vector<std::vector<uint32_t>> lst(nt);
  std::vector<uint32_t> order(e->dtp.size());
  for (uint32_t d = 0; d < order.size(); d++) order[d] = d;
  std::stable_sort(order.begin(), order.end(),
                   [&](uint32_t a, uint32_t b) { return e->dtp[a].track < e->dtp[b].track; });
  for (uint32_t d : order)
    if (e->dtp[d].ext_transport_cc && e->dtTransport[d] >= 0) lst[size_t(e->dtTransport[d])].push_back(d);
  std::vector<uint32_t> off(nt + 1, 0), flat;
  for (uint32_t t = 0; t < nt; t++) {
    off[t] = uint32_t(flat.size());
    flat.insert(flat.end(), lst[t].begin(), lst[t].end());
  }
  off[nt] = uint32_t(flat.size());
  // grow the transport counters (first: before any transport), keeping the old ones
  // (both new buffers first: a failed allocation leaves the old counters and offsets as they were)
  if (nt > e->dTwccCtrT.cap() || !e->dTwccCtrT) {
    const uint32_t old = uint32_t(e->dTwccCtrT.cap());
    const uint32_t cap = std::max<uint32_t>(nt, 2 * old + 64);
    DevBuf<uint32_t> c, o;
    HIPCHK(c.alloc(cap), "alloc twcc counters");
    HIPCHK(o.alloc(cap + 1), "alloc twcc offsets");
    HIPCHK(hipMemset(c, 0, size_t(cap) * sizeof(uint32_t)), "twcc counters reset");
    if (e->dTwccCtrT)
      HIPCHK(hipMemcpy(c, e->dTwccCtrT, size_t(old) * sizeof(uint32_t), hipMemcpyDeviceToDevice),
             "twcc counters move");
    e->dTwccCtrT = std::move(c);
    e->dTwccTOff = std::move(o);
  }
  HIPCHK(e->dTwccTList.reserve(std::max<size_t>(flat.size(), 1), 1024), "alloc twcc lists");  // (allocated even when empty)
  HIPCHK(hipMemcpy(e->dTwccTOff, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "twcc offsets");
  if (!flat.empty())
    HIPCHK(hipMemcpy(e->dTwccTList, flat.data(), flat.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "twcc lists");
  e->nTwccT = nt;
  e->twccDirty = false;
  return upload_done(e);
}

// ---- lkf_run: its stages in the order they run -----------------------------
using clk = std::chrono::steady_clock;
static double ms_between(clk::time_point a, clk::time_point b) {
  return std::chrono::duration<double, std::milli>(b - a).count();
}
static double ms_since(clk::time_point a) { return ms_between(a, clk::now()); }

// What the stages of one lkf_run share.
struct RunCtx {
  int ci;               // the batch context's index
  uint32_t nt, nd, nl;  // tracks, DownTracks, schedule lanes
  Event *rg;            // this run's timing events
  bool keyed;           // the run has keyed control ops
  bool prepDone;        // an ingest's k_ing_out prepared the batch (no k_batch_init / k_track_ranges)
  bool ingestFed;       // the batch is an ingest's output (emit's residency)
  size_t nev;           // control ops staged
  clk::time_point tp0, tp1, tp2, tp25, tp3;  // LKF_HOST_PROF sections
};

// A track's layer-offset changes: one op per active DownTrack of it.
static void expand_track_ops(lkf_engine *e, const RunCtx &r) {
  if (e->trkOps.empty()) return;
  auto trk_key = [](const lkf_engine::TrackOp &o) {
    lkf_engine::Pend q;
    q.ev.at = o.at;
    q.key = o.key;
    q.kind = o.kind;
    return ctl_sort_key(q);
  };
  std::stable_sort(e->trkOps.begin(), e->trkOps.end(),
                   [&](const lkf_engine::TrackOp &a, const lkf_engine::TrackOp &b) {
                     return a.track != b.track ? a.track < b.track : trk_key(a) < trk_key(b);
                   });
  std::vector<std::vector<uint32_t>> byT(r.nt);
  for (uint32_t d = 0; d < r.nd; d++)
    if (e->active[d]) byT[e->dtp[d].track].push_back(d);
  for (const auto &op : e->trkOps) {
    lkf_engine::Pend q;
    std::memset(&q.ev, 0, sizeof(q.ev));
    q.ev.at = op.at;
    q.key = op.key;
    q.kind = op.kind;
    q.ev.op = kOpLayerOffsets;
    for (int k = 0; k < 4; k++) q.ev.a[k] = int64_t(uint64_t(op.offs[2 * k]) | (uint64_t(op.offs[2 * k + 1]) << 32));
    q.ev.pad = int64_t(op.offs[8]);
    for (uint32_t d : byT[op.track]) {
      q.dt = d;
      e->pending.push_back(q);
    }
  }
}

// Keyed ops: a DownTrack's in-batch ops must all be of one kind (its
// positions resolve in one space, and its lane stays sorted by at_pkt).
// Nothing of this run is enqueued yet: the ops are dropped, the batch stays.
static int refuse_mixed_kinds(lkf_engine *e, const RunCtx &r) {
  const int64_t bad = e->csr.mixed(e->pending.data(), e->pending.size(), e->dtLane.data(), r.nd);
  if (bad < 0) return LKF_OK;
  char buf[160];
  snprintf(buf, sizeof(buf), "DownTrack %lld: control ops of two position kinds (lkf_at_kind) in one run",
           (long long)bad);
  e->err = buf;
  e->pending.clear();
  e->trkOps.clear();
  return LKF_EINVAL;
}

// The prep stream waits for the batch's inputs (the caller's stream, an
// ingest) and for this context's previous batch; what kind of batch this is.
static int wait_inputs(lkf_engine *e, BatchCtx &x, RunCtx &r, hipStream_t us) {
  hipStream_t ps = e->prepS;
  HIPCHK(hipEventRecord(e->inEv, us), "event");
  HIPCHK(hipStreamWaitEvent(ps, e->inEv, 0), "wait caller stream");
  // this context's previous batch (run n-2) must have finished its emit stage
  if (x.used) HIPCHK(hipStreamWaitEvent(ps, x.emitted, 0), "wait emit");
  if (x.fromIngest && e->haveBatch) HIPCHK(hipStreamWaitEvent(ps, x.ingested, 0), "wait ingest");
  r.prepDone = x.fromIngest && e->haveBatch && x.prepByIngest && x.prepNT == r.nt && x.prepND == r.nd &&
               e->curPkts == x.dPktsOwn;
  r.ingestFed = x.fromIngest && e->haveBatch;
  x.fromIngest = false;
  x.prepByIngest = false;
  return LKF_OK;
}

// Per-lane control-op CSR (stable: queue order within a lane, then by
// key: at_pkt, or a keyed op's datagram index / arrival time).  The host
// sorts only the ops: an LSD radix sort on the lane (8-bit digits, stable),
// then a stable insertion by key inside a lane with several ops; it stages
// the run's RunDesc, the sorted ops, their lanes and — in a run with keyed
// ops — their keys in this context's page-locked cached buffer.  The prep stage's
// first kernel pulls them and k_ev_offsets derives the dense per-lane
// offsets on the GPU (no host pass over all lanes).
static int stage_ctl(lkf_engine *e, BatchCtx &x, RunCtx &r) {
  r.tp1 = clk::now();
  if (x.used) HIPCHK(hipEventSynchronize(x.pulled), "stage wait");  // run n-3's pull of this staging is done
  if (x.used && x.keyed) HIPCHK(hipEventSynchronize(x.prepped), "stage wait (keys)");  // ... and its resolver
  x.keyed = r.keyed;
  r.tp2 = clk::now();
  const size_t nev = r.nev = e->csr.sort(e->pending.data(), e->pending.size(), e->dtLane.data(), r.nl);  // (ctl_csr.h)
  if (nev > x.stageCap || !x.stage.host) {  // (graphs captured with the old staging are re-captured)
    // the queued pull of this context's previous run may still read the old
    // staging, and its graphs are destroyed when re-captured: drain first
    if (x.stage.host) {
      if (int rc = drain_streams(e)) return rc;
    }
    x.stage.reset();
    x.stageCap = 0;  // (set once the allocation has succeeded: a failed one is retried by the next run)
    // (a multiple of 4 ops: the keys behind the lane list stay 16-B aligned)
    const uint32_t cap = uint32_t(std::max<size_t>(2 * nev, 4096) + 3) & ~3u;
    HIPCHK(x.stage.alloc(stage_bytes(cap)), "alloc stage");
    x.stageCap = cap;
    x.forget_pull_graphs();
  }
  // (the keys of a run with keyed ops: behind the lane list, read in place by k_ev_resolve)
  uint8_t *h = x.stage.host;
  e->csr.emit(e->pending.data(), reinterpret_cast<DevEvent *>(h + stage_ev_off(x.stageCap)),
              reinterpret_cast<uint32_t *>(h + stage_lane_off(x.stageCap)),
              r.keyed ? reinterpret_cast<DevKey *>(h + stage_key_off(x.stageCap)) : nullptr, e->dtp.data());
  e->pending.clear();
  {
    RunDesc &d = *reinterpret_cast<RunDesc *>(h);
    std::memset(&d, 0, sizeof(d));
    d.pkts = reinterpret_cast<uint64_t>(e->curPkts);
    d.arena = reinterpret_cast<uint64_t>(e->curArena);
    d.dd = reinterpret_cast<uint64_t>(e->curDD);
    d.nDev = reinterpret_cast<uint64_t>(e->curNDev);
    d.n = e->curN;
    d.nev = uint32_t(nev);
    d.evCap = x.stageCap;
  }
  r.tp25 = clk::now();
  if (nev > x.dEvents.cap() || size_t(r.nl) + 1 > x.dEvOff.cap() || nev > x.dEvLane.cap()) {
    // this context's op buffers: its previous run (n-3) must be done with them.
    // ps waits on that run's "emitted" event above, so draining ps covers its
    // prep, decide and emit stages (the lane list is read by k_ev_offsets on ps,
    // the ops and offsets by the decide stage).
    // (every stream: the pull graph on the engine's own stream reads them too,
    // and the graphs captured with them are destroyed below)
    if (int rc = drain_streams(e)) return rc;
    if (nev > x.dEvents.cap()) HIPCHK(x.dEvents.reserve(2 * nev, 4096), "alloc events");
    if (size_t(r.nl) + 1 > x.dEvOff.cap()) HIPCHK(x.dEvOff.alloc(size_t(r.nl) + 1 + 4096), "alloc evoff");
    if (nev > x.dEvLane.cap()) HIPCHK(x.dEvLane.reserve(2 * nev, 4096), "alloc evlane");
    x.forget_pull_graphs();
  }
  r.tp3 = clk::now();
  return LKF_OK;
}

// A stage's launches on stream st (pull_body, prep_body, scan_tail).
using StageBody = int (*)(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t st);

// (Re)captures a stage as a graph on stream st: the captured launches are the
// same as the direct ones.
static int capture_stage(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t st, GraphExec &g, StageBody body) {
  // an exec is destroyed only once its last launch (on st, this context's
  // previous run) has finished: HIP may release its kernel arguments at once
  if (g) {
    HIPCHK(hipStreamSynchronize(st), "graph idle");
    HIPCHK(g.destroy(), "graph destroy");
  }
  HIPCHK(hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed), "begin capture");
  const int rc = body(e, x, r, st);
  hipGraph_t graph = nullptr;
  const hipError_t re = hipStreamEndCapture(st, &graph);
  if (rc) return rc;
  HIPCHK(re, "end capture");
  const hipError_t ri = hipGraphInstantiate(&g.h, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  HIPCHK(ri, "graph instantiate");
  return LKF_OK;
}

// One stage on stream st: its graph, re-captured when the topology epoch moved
// (or nothing is captured yet), or — LKF_GRAPH=0 — body's launches directly.
static int run_stage(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t st, StageGraph &g, StageBody body,
                     const char *what) {
  if (!e->knobs.useGraph) return body(e, x, r, st);
  if (g.epoch != e->epoch || !g.exec) {
    if (int rc = capture_stage(e, x, r, st, g.exec, body)) return rc;
    g.epoch = e->epoch;
  }
  HIPCHK(hipGraphLaunch(g.exec, st), what);
  return LKF_OK;
}

// the control-op pull (k_h2d: the run descriptor and the ops from the
// pinned staging; k_ev_offsets)
static int pull_body(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t cs) {
  HIPCHK(launch_h2d(cs, x.stage.dev, x.dDesc, x.dEvents, x.dEvLane), "event pull");
  HIPCHK(launch_ev_offsets(cs, x.dEvLane, x.dDesc, r.nl, x.dEvOff), "event offsets");
  return LKF_OK;
}

static int prep_body(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t ps) {
  const uint32_t nt = r.nt, nd = r.nd;
  if (!r.prepDone) {  // (an ingest's k_ing_out did both)
    HIPCHK(launch_batch_init(ps, nt, nd, kStatsWords * (1 + kStatCopies), x.dTBegin, x.dTEnd, x.dTRuns, x.dErr,
                             x.dStats, x.dFwdCnt, x.dFwdBytes),
           "batch init");
    HIPCHK(launch_track_ranges(ps, x.dDesc, e->cfg.max_batch_pkts, nt, x.dTBegin, x.dTEnd, x.dTRuns, x.dErr),
           "track_ranges");
  }
  HIPCHK(launch_scan(ps, 0, e->dDTs, x.dTBegin, x.dTEnd, nullptr, nullptr, nd, x.dPartA, nullptr, x.dSlotBase,
                     nullptr, x.dTot + 0, nullptr, nullptr),
         "slot scan");
  HIPCHK(launch_layer_index(ps, x.dDesc, x.dTBegin, x.dTEnd, nt, e->cfg.max_batch_pkts, x.dLayerList,
                            x.dLayerBefore, x.dLayerCnt, e->ddAlloc ? x.dDDUsed : nullptr),
         "layer index");
  if (e->nTrk)  // StreamTracker.Observe of every (track, spatial layer) tracker (receiver.go:686-695)
    HIPCHK(launch_tracker_observe(ps, e->dTrk, e->nTrk, x.dDesc, x.dTBegin, x.dTEnd), "tracker observe");
  if (e->ddAlloc) {  // dependency descriptors of this batch (track structure rings advance in order)
    HIPCHK(launch_dd_decode(ps, x.dDesc, x.dTBegin, x.dTEnd, e->dTracks, nt, e->dDDStruct, e->dDDTrack, x.dDDPkt,
                            x.dErr, e->nDDTrk ? e->dTrackDDTrk : nullptr, e->dDDTrk, x.dDDSpill,
                            reinterpret_cast<uint32_t *>(x.dDDUsed + 1), uint32_t(x.dDDSpill.cap())),
           "dd decode");
  }
  return LKF_OK;
}

// ---- prep stage (prep stream): the pull, per-batch init, track ranges,
// slot scan, layer index, tracker observe, DD decode, key resolve
static int enqueue_prep(lkf_engine *e, BatchCtx &x, const RunCtx &r) {
  hipStream_t ps = e->prepS;
  if (!e->ingestStarted) HIPCHK(hipEventRecord(r.rg[0], ps), "event");  // else: recorded ahead of the ingest
  e->ingestStarted = false;
  // the control-op pull on the engine's own stream: it does not depend on the
  // batch, so it runs beside a preceding ingest instead of after it on the
  // prep stream
  hipStream_t cs = e->own;
  if (x.used) HIPCHK(hipStreamWaitEvent(cs, x.emitted, 0), "wait emit (pull)");
  if (int rc = run_stage(e, x, r, cs, x.gCtl, pull_body, "pull graph")) return rc;
  HIPCHK(hipEventRecord(x.pulled, cs), "event");
  HIPCHK(hipStreamWaitEvent(ps, x.pulled, 0), "wait pull");
  StageGraph &gPrep = x.gPrep[r.prepDone ? 1 : 0];
  if (int rc = run_stage(e, x, r, ps, gPrep, prep_body, "prep graph")) return rc;
  if (r.keyed && r.nev) {
    // Keyed ops -> ExtPacket indices (DevEvent.at), after the pull and the
    // track ranges, before the decide stage reads the ops.  Launched directly
    // and only for a run with keyed ops: a run without them enqueues what it
    // always did.
    const bool scan = e->curFromIngest && e->curNDev;  // (an empty ingest: every datagram key is past it)
    HIPCHK(launch_ev_resolve(ps, reinterpret_cast<const DevKey *>(x.stage.dev + stage_key_off(x.stageCap)), x.dEvents,
                             x.dEvLane, uint32_t(r.nev), e->curPkts, x.dTBegin, x.dTEnd, r.nt,
                             scan ? e->dPos.get() : nullptr, e->curFromIngest ? e->lastIngestN : 0xffffffffu),
           "key resolve");
    if (scan) {
      HIPCHK(hipEventRecord(e->scanRead, ps), "event");
      e->scanReadPending = true;
    }
  }
  HIPCHK(hipEventRecord(x.prepped, ps), "event");
  if (e->knobs.debugDD && e->ddAlloc) {  // LKF_DEBUG_DD=1 (diagnostic): the context's DD cursor after its prep
    HIPCHK(hipStreamSynchronize(ps), "debug sync");
    uint64_t u[2] = {0, 0};
    HIPCHK(hipMemcpy(u, x.dDDUsed, sizeof(u), hipMemcpyDeviceToHost), "debug copy");
    fprintf(stderr, "[lkf dd] run %llu ctx %d after prep: cursor %llu spill %llu graph %d epoch %llu/%llu\n",
            (unsigned long long)e->nRuns, r.ci, (unsigned long long)u[0], (unsigned long long)u[1],
            int(e->knobs.useGraph), (unsigned long long)gPrep.epoch, (unsigned long long)e->epoch);
  }
  return LKF_OK;
}

// Several DownTracks per decide wave when the batch is short (a 10-20 ms
// tick has a few packets per track): the per-DownTrack prologue then
// dominates and one workgroup per DownTrack is dispatch-rate bound.
static uint32_t decide_per_wave(const lkf_engine *e, const RunCtx &r) {
  if (e->knobs.decideK) return e->knobs.decideK;
  // (round 6: 2 below 48 packets per track — 4 at the shortest ticks measured
  // slower since the stream wave and the NACK queues changed: 10-ms ticks at
  // 1,000 rooms 0.555 -> 0.533 ms ingress, 0.338 -> 0.331 ms ExtPacket, at 100
  // rooms 0.130 -> 0.106 ms; 1: 0.557 / 0.346 ms; profiles/r6_ab_runs.txt)
  // Many DownTracks: one wave each is bound by the dispatch rate (≈240 waves
  // per µs over the 8 XCDs: configs[2]'s 337 k DownTracks ≈ 1.4 ms), so a
  // wave serves one more DownTrack per 100 k (configs[2] 2.74 -> 2.54 ms at
  // 4; configs[1]'s 18 k stay at one: 2 costs 0.74 -> 0.87 ms there;
  // configs[3]'s 100 k measured alike at 1 and 2)
  const uint64_t per = uint64_t(e->curN) / std::max<uint32_t>(1, r.nt);  // (ingest: the datagram count bound)
  const uint32_t byCount = uint32_t(std::min<uint64_t>(8, (uint64_t(r.nd) + 99999) / 100000));
  return std::max<uint32_t>(per >= 48 ? 1 : 2, byCount);
}

static DecideArgs decide_args(const lkf_engine *e, const BatchCtx &x, const RunCtx &r) {
  DecideArgs d{};
  d.layerList = x.dLayerList;
  d.layerBefore = x.dLayerBefore;
  d.layerCnt = x.dLayerCnt;
  d.pktStride = e->cfg.max_batch_pkts;
  d.sched = e->dSched;
  d.waveTrack = e->dWaveTrack;
  d.nlanes = r.nl;
  d.hot = e->dHot;
  d.dts = e->dDTs;
  d.tracks = e->dTracks;
  d.rm = e->dRm;
  d.vc = e->dVc;
  d.seq = e->dSeq;
  d.seqSize = e->cfg.seq_size;
  d.srm = e->dSrm;
  d.srmStride = e->srmStride;
  d.srmCap = e->srmCap;
  d.pkts = e->curPkts;
  d.tBegin = x.dTBegin;
  d.tEnd = x.dTEnd;
  d.slotBase = x.dSlotBase;
  d.recs = x.dRecs;
  d.fbase = x.dFBase;
  d.wide = x.dWide;
  d.ss = e->dSS;
  d.ssRing = e->dSSRing;
  d.ssGap = e->dSSGap;
  d.dtOffs = e->dDTOffs;
  d.tupleCap = e->cfg.max_batch_tuples;
  d.err = x.dErr;
  d.events = x.dEvents;
  d.evOff = x.dEvOff;
  d.fwdCnt = x.dFwdCnt;
  d.fwdBytes = x.dFwdBytes;
  d.dtCum = e->dDTCum;
  d.stats = x.dStats;
  d.perWave = decide_per_wave(e, r);
  d.ddPkts = e->ddAlloc ? x.dDDPkt.get() : nullptr;
  d.ddStructs = e->dDDStruct;
  d.ddState = e->ddAlloc ? e->dDDState.get() : nullptr;
  d.ddArena = x.dDDArena;
  d.ddUsed = x.dDDUsed;
  d.ddSpill = e->ddAlloc ? x.dDDSpill.get() : nullptr;
  d.ddCap = x.dDDArena.cap();
  d.maxDts = e->cfg.max_downtracks;
  d.maxTracks = e->cfg.max_tracks;
  d.npkts = e->curN;  // (an ingest-produced batch: the launch bound)
  d.nev = uint32_t(r.nev);
  return d;
}

static int scan_tail(lkf_engine *e, BatchCtx &x, const RunCtx &r, hipStream_t st) {
  // counters and the output scan stay on the (high-priority) decide stream:
  // on the low-priority emit stream these small kernels queued behind the
  // next batch's decide waves and were on the emit chain's critical path
  HIPCHK(launch_stats_reduce(st, x.dStats), "stats reduce");
  HIPCHK(launch_scan(st, 1, e->dDTs, nullptr, nullptr, x.dFwdCnt, x.dFwdBytes, r.nd, x.dPartA, nullptr, x.dRecBase,
                     x.dByteBase, x.dTot + 2, x.dTot + 3, e->dPerm, x.dGFirst, e->cfg.max_out_pkts),
         "out scan");
  return LKF_OK;
}

// ---- decide stage (decide stream): decide, its counters and output scan,
// the transport-cc bases, the sequencer's DD bytes
static int enqueue_decide(lkf_engine *e, BatchCtx &x, const RunCtx &r) {
  hipStream_t s = e->decS;
  HIPCHK(hipStreamWaitEvent(s, x.prepped, 0), "wait prep");
  const DecideArgs d = decide_args(e, x, r);
  HIPCHK(hipEventRecord(r.rg[1], s), "event");
  HIPCHK(launch_decide(s, d, e->ddLanes), "decide");
  HIPCHK(hipEventRecord(r.rg[2], s), "event");
  if (int rc = run_stage(e, x, r, s, x.gScan, scan_tail, "scan graph")) return rc;
  if (e->anyTwcc)  // the transports' sequence ranges of this batch (after the forwarded counts)
    HIPCHK(launch_twcc_base(s, e->dDTs, r.nd, x.dFwdCnt, e->dTwccCtrD, e->dTwccCtrT, e->dTwccTOff, e->dTwccTList,
                            e->nTwccT, x.dTwccBase),
           "twcc base");
  HIPCHK(hipEventRecord(x.decided, s), "event");
  if (e->nSeqDD && e->ddAlloc) {  // sequencer ddBytes (decide stream: before the next batch's decide)
    SeqDDLaunch q;
    q.list = e->dSeqDDList;
    q.n = e->nSeqDD;
    q.hot = e->dHot;
    q.seq = e->dSeq;
    q.seqSize = e->cfg.seq_size;
    q.srm = e->dSrm;
    q.srmStride = e->srmStride;
    q.srmCap = e->srmCap;
    q.ddIdx = e->dSeqDDIdx;
    q.seqDD = e->dSeqDD;
    q.recs = x.dRecs;
    q.fbase = x.dFBase;
    q.wide = x.dWide;
    q.slotBase = x.dSlotBase;
    q.fwdCnt = x.dFwdCnt;
    q.pkts = e->curPkts;
    q.ddArena = x.dDDArena;
    HIPCHK(launch_seq_dd(s, q), "sequencer dd");
  }
  return LKF_OK;
}

static EmitArgs emit_args(const lkf_engine *e, const BatchCtx &x, const RunCtx &r) {
  EmitArgs m{};
  m.perm = e->dPerm;
  m.recBase = x.dRecBase;
  m.byteBase = x.dByteBase;
  m.gFirst = x.dGFirst;
  m.slotBase = x.dSlotBase;
  m.totals = x.dTot + 2;
  m.recs = x.dRecs;
  m.fbase = x.dFBase;
  m.wide = x.dWide;
  m.pkts = e->curPkts;
  m.arena = e->curArena;
  m.dts = e->dDTs;
  m.ndts = r.nd;
  m.out = x.dOut;
  m.outArena = x.dOutArena;
  m.outCap = e->cfg.max_out_pkts;
  m.outByteCap = e->cfg.max_out_bytes;
  m.err = x.dErr;
  m.ddArena = e->ddAlloc ? x.dDDArena.get() : nullptr;
  m.maxDts = e->cfg.max_downtracks;
  m.npkts = e->curN;
  m.tupleCap = e->cfg.max_batch_tuples;
  m.arenaLen = e->curArenaLen;
  m.ddCap = x.dDDArena.cap();
  m.twccBase = e->anyTwcc ? x.dTwccBase.get() : nullptr;
  m.gCap = e->cfg.max_out_pkts / 64 + 2;
  return m;
}

// One workgroup per 64-record group (grid = the capacity bound; workgroups
// past the batch's records exit at once).  Short-lived workgroups free their
// slots as they finish, so the next batch's decide stage (higher-priority
// stream) interleaves with this emit instead of waiting for a persistent grid.
static uint32_t emit_grid(const lkf_engine *e) {
  return e->knobs.emitPersistent ? e->emitGrid : uint32_t(((e->cfg.max_out_pkts + 63) / 64 + 7) / 8 * 8);
}

// An ingest-fed batch's emit runs beside the next ingest chain: at a low
// fan-out (fewer than emitCapFanout DownTracks per track) its workgroups are
// capped at 12 per CU (LDS reserved at launch), which keeps the payload lines
// its DownTracks re-read in L2 and leaves CUs to the ingest (configs[1], 9 per
// track: 0.78 -> 0.74 ms per step).  A submitted batch's emit, or one with a
// high fan-out, is most of the step and runs uncapped (the cap: ExtPacket
// configs[1] 0.455 -> 0.54 ms, configs[2] 2.51 -> 2.83 ms, configs[3] 3.35 ->
// 3.47 ms; profiles/r6_ab_runs.txt).
static uint32_t emit_lds_pad(const lkf_engine *e, const RunCtx &r) {
  const bool lowFanout = uint64_t(r.nd) < uint64_t(e->knobs.emitCapFanout) * std::max<uint32_t>(1, r.nt);
  return r.ingestFed && lowFanout ? e->knobs.emitLdsPad : 0;
}

// ---- emit stage (emit stream): wire bytes.  The decide stream goes
// straight on to the next batch's decide.
static int enqueue_emit(lkf_engine *e, BatchCtx &x, const RunCtx &r) {
  hipStream_t es = e->emitS;
  HIPCHK(hipStreamWaitEvent(es, x.decided, 0), "wait decided");
  HIPCHK(hipEventRecord(r.rg[3], es), "event");
  const EmitArgs m = emit_args(e, x, r);
  const uint32_t grid = emit_grid(e);
  x.egress = e->egress;
  if (x.egress == LKF_EGRESS_PREFIX) {  // records + prefixes only (three launches, no payload traffic)
    EmitPrefixLaunch q;
    q.pre = x.dPre;
    q.gSum = x.dPreGSum;
    q.gBase = x.dPreGBase;
    q.total = x.dPreTot;
    if (r.nd)
      HIPCHK(launch_emit_prefix(es, m, grid, q), "emit prefix");
    else
      HIPCHK(hipMemsetAsync(x.dPreTot, 0, sizeof(uint64_t), es), "emit prefix");
  } else if (r.nd) {
    HIPCHK(launch_emit(es, m, grid, emit_lds_pad(e, r)), "emit");
  }
  HIPCHK(hipEventRecord(r.rg[4], es), "event");
  HIPCHK(launch_accumulate(es, x.dStats, x.dTot, e->dCum, x.dErr, e->dSticky), "accumulate");
  // (sendingPacket -> RTPStatsSender.Update of every forwarded tuple runs inside
  // decide, ss_fold.)  This batch's bucket copies (sender stream) finish before
  // its context counts as done.
  if (e->bktStorePending) {
    HIPCHK(hipEventRecord(x.sent, e->sendS), "event");
    HIPCHK(hipStreamWaitEvent(es, x.sent, 0), "wait bucket store");
  }
  e->bktStorePending = false;
  HIPCHK(hipEventRecord(x.emitted, es), "event");
  return LKF_OK;
}

// End-of-run bookkeeping: the host profile, then the engine moves on to the
// next context.
static void finish_run(lkf_engine *e, BatchCtx &x, const RunCtx &r) {
  if (e->knobs.hostProf && e->nRuns >= 3) {  // steady state: skip the first runs (initial control ops, first touch)
    e->hp[0] += ms_between(r.tp0, r.tp1);
    e->hp[1] += ms_between(r.tp1, r.tp2);
    e->hp[2] += ms_between(r.tp2, r.tp25);
    e->hp[6] += ms_between(r.tp25, r.tp3);
    e->hp[3] += ms_since(r.tp3);
    e->hp[4] += ms_since(r.tp0);
    e->hp[5] += 1;
  }
  x.used = true;
  x.protectedRun = false;
  if (!e->protRun.empty()) e->protRun[e->nRuns % 256] = 0;
  e->lastCtx = r.ci;
  e->nRuns++;
  e->haveBatch = false;
  e->curNDev = nullptr;
  e->curDD = nullptr;
}

int lkf_run(lkf_engine *e, void *stream) {
  if (!e) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (int rc = flush_topology(e)) return rc;
  if (e->schedDirty) {
    if (int rc = rebuild_sched(e)) return rc;
  }
  if (e->twccDirty) {
    if (int rc = rebuild_twcc(e)) return rc;
  }
  RunCtx r{};
  r.ci = int(e->nRuns % lkf_engine::kCtx);
  BatchCtx &x = e->ctx[r.ci];
  if (!e->haveBatch) {  // control-only run: an empty batch applies queued ops
    e->curPkts = x.dPktsOwn;
    e->curArena = x.dArenaOwn;
    e->curOwned = e->curDDOwned = true;
    e->curN = 0;
    e->curNDev = nullptr;
    e->curArenaLen = 0;
    e->curFromIngest = false;
  }
  // The caller's stream orders the batch's inputs; the stages themselves run
  // on the engine's streams (completion: lkf_sync).  The prep stream (the
  // control-op CSR's offsets, per-batch init, track ranges, slot scan, layer
  // index and, before lkf_run, the ingest) runs ahead: batch n+1 is prepared
  // while batch n decides, so decide(n+1) starts as soon as decide(n) ends.
  r.tp0 = clk::now();
  hipStream_t us = stream ? reinterpret_cast<hipStream_t>(stream) : e->own;
  e->cur = us;
  r.nt = uint32_t(e->tracks.size());
  r.nd = uint32_t(e->dtp.size());
  r.nl = uint32_t(e->sched.size());
  r.rg = e->ring[e->nRuns % lkf_engine::kRing];
  expand_track_ops(e, r);
  r.keyed = e->keyedPending;
  e->keyedPending = false;
  if (r.keyed) {
    if (int rc = refuse_mixed_kinds(e, r)) return rc;
  }
  for (const auto &op : e->trkOps)
    std::memcpy(e->tracks[op.track].layer_offsets, op.offs, sizeof(op.offs));  // as of the end of this run
  e->trkOps.clear();
  if (int rc = wait_inputs(e, x, r, us)) return rc;
  if (int rc = stage_ctl(e, x, r)) return rc;
  if (int rc = enqueue_prep(e, x, r)) return rc;
  if (int rc = enqueue_decide(e, x, r)) return rc;
  if (int rc = enqueue_emit(e, x, r)) return rc;
  finish_run(e, x, r);
  return LKF_OK;
}

// Waits for all queued batches; reports (and clears) the sticky error word:
// every error of every batch and ingest since the last lkf_sync.
int lkf_sync(lkf_engine *e) {
  if (!e) return LKF_EINVAL;
  int rc = drain_streams(e);
  if (rc) return rc;
  uint32_t acc = 0;
  D2H(&acc, e->dSticky, sizeof(acc), "err copy");
  if (e->knobs.debugDD && e->ddAlloc) {
    for (int c = 0; c < lkf_engine::kCtx; c++) {
      uint64_t u[2] = {0, 0};
      if (hipMemcpy(u, e->ctx[c].dDDUsed, sizeof(u), hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "[lkf dd] sync after run %llu: ctx %d cursor %llu (%p)\n", (unsigned long long)e->nRuns, c,
                (unsigned long long)u[0], static_cast<void *>(e->ctx[c].dDDUsed));
    }
  }
  if (!acc) return LKF_OK;
  HIPCHK(hipMemset(e->dSticky, 0, sizeof(uint32_t)), "err reset");
  HIPCHK(hipDeviceSynchronize(), "err reset sync");  // null-stream memset vs the engine's streams
  if (acc & (3u << 8)) {
    e->err = "raw batch not grouped by track / bad stream handle";
    return LKF_EORDER;
  }
  if (acc & (4u << 8)) {
    e->err = "dependency descriptor beyond an engine limit (templates, frame diffs, chains)";
    return LKF_ENOSPC;
  }
  if (acc & (8u << 8)) {
    e->err = "RTCP NACK pair capacity of an ingest exceeded";
    return LKF_ENOSPC;
  }
  if (acc & 32u) {
    e->err = "internal: a DownTrack with padding exclusions was decided by the plain kernel";
    return LKF_EINVAL;
  }
  if (acc & 16u) {
    e->err = "dependency descriptor unreadable, missing its lkf_pkt_dd entry, or beyond an engine limit";
    return LKF_EINVAL;
  }
  if (acc & 3u) {
    e->err = "batch not grouped by track / bad track handle";
    return LKF_EORDER;
  }
  if (acc & 64u) {
    e->err = "output or tuple capacity exceeded (decide: the batch's DD arena)";
    if (e->ddAlloc) {  // (the contexts' cursors, for the report)
      char buf[192];
      size_t o = 0;
      for (auto &x : e->ctx) {
        uint64_t u[2] = {0, 0};
        if (x.dDDUsed && hipMemcpy(u, x.dDDUsed, sizeof(u), hipMemcpyDeviceToHost) == hipSuccess && o < sizeof(buf))
          o += size_t(snprintf(buf + o, sizeof(buf) - o, " %llu/%llu", (unsigned long long)u[0],
                               (unsigned long long)x.dDDArena.cap()));
      }
      e->err += " used/cap:";
      e->err += buf;
      // (diagnostic) the live allocations around context 0's cursor, and the
      // contexts' small buffers by name
      const uintptr_t c0 = reinterpret_cast<uintptr_t>(e->ctx[0].dDDUsed.get());
      {
        std::lock_guard<std::mutex> g(dreg().m);
        for (auto it = dreg().a.lower_bound(c0 > (1u << 20) ? c0 - (1u << 20) : 0);
             it != dreg().a.end() && it->first < c0 + (1u << 20); ++it) {
          char t[64];
          snprintf(t, sizeof(t), " [%+lld:%zu]", (long long)(intptr_t(it->first) - intptr_t(c0)), it->second);
          e->err += t;
        }
      }
      for (int c = 0; c < lkf_engine::kCtx; c++) {
        const BatchCtx &x = e->ctx[c];
        const void *ps[] = {x.dTBegin, x.dTEnd, x.dTRuns, x.dErr, x.dTot, x.dDesc, x.dEvents, x.dEvOff, x.dEvLane,
                            x.dDDUsed, x.dStats, x.dPartA, x.dFBase, x.dLayerCnt, x.dTwccBase};
        const char *nm[] = {"tB", "tE", "tR", "err", "tot", "desc", "ev", "evoff", "evlane", "ddu", "stats",
                            "partA", "fbase", "lcnt", "twcc"};
        for (size_t k = 0; k < sizeof(ps) / sizeof(ps[0]); k++) {
          const intptr_t dlt = intptr_t(reinterpret_cast<uintptr_t>(ps[k])) - intptr_t(c0);
          if (ps[k] && dlt > -(1 << 20) && dlt < (1 << 20)) {
            char t[48];
            snprintf(t, sizeof(t), " %d.%s%+lld", c, nm[k], (long long)dlt);
            e->err += t;
          }
        }
      }
    }
    return LKF_ENOSPC;
  }
  if (acc & 12u) {
    e->err = (acc & 8u) ? "output or tuple capacity exceeded (decide: tuple slots)"
                        : "output or tuple capacity exceeded (emit: output records or bytes)";
    return LKF_ENOSPC;
  }
  return LKF_OK;
}

int lkf_get_stats(lkf_engine *e, lkf_stats *out) {
  if (!e || !out) return LKF_EINVAL;
  std::memset(out, 0, sizeof(*out));
  int rc = lkf_sync(e);
  if (e->lastCtx < 0) return rc;
  BatchCtx &x = e->ctx[e->lastCtx];
  uint64_t st[kStatsWords];
  uint64_t tot[4];
  D2H(st, x.dStats, sizeof(st), "stats copy");
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  out->tuples = st[0];
  out->forwarded = st[1];
  out->out_bytes = st[2];
  out->arena_bytes = tot[3];
  for (int i = 0; i < LKF_DROP_NREASONS; i++) out->drops[i] = st[4 + i];
  return rc;
}

// The accessors of one egress mode refuse a run enqueued in the other.
static int egress_is(lkf_engine *e, const BatchCtx &x, int mode) {
  if (x.egress == mode) return LKF_OK;
  e->err = mode == LKF_EGRESS_WIRE
               ? "the run was enqueued in prefix egress mode: read it with lkf_drain_prefix* / lkf_output_prefix_device"
               : "the run was enqueued in wire egress mode: read it with lkf_drain* / lkf_output_device";
  return LKF_EINVAL;
}

int lkf_set_egress(lkf_engine *e, int mode) {
  if (!e) return LKF_EINVAL;
  if (mode != LKF_EGRESS_WIRE && mode != LKF_EGRESS_PREFIX) {
    e->err = "unknown egress mode";
    return LKF_EINVAL;
  }
  if (mode == LKF_EGRESS_PREFIX) {
    HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
    const uint64_t groups = e->cfg.max_out_pkts / 64 + 2;
    for (auto &x : e->ctx) {
      const bool ok = (x.dPre || !x.dPre.alloc(e->cfg.max_out_pkts)) && (x.dPreGSum || !x.dPreGSum.alloc(groups)) &&
                      (x.dPreGBase || !x.dPreGBase.alloc(groups)) && (x.dPreTot || !x.dPreTot.alloc(1));
      if (!ok) {
        (void)hipGetLastError();
        e->err = "prefix egress: out of device memory for the record buffers";
        return LKF_ENOMEM;
      }
    }
  }
  e->egress = mode;
  return LKF_OK;
}

// The prefix accessors' common part: the run of context x was a prefix-mode
// run within the engine's capacity -> its record count and prefix arena bytes.
static int prefix_totals(lkf_engine *e, BatchCtx &x, uint64_t *n_out, uint64_t *arena_len) {
  const int rc = egress_is(e, x, LKF_EGRESS_PREFIX);
  if (rc) return rc;
  uint64_t tot[4], pre = 0;
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  D2H(&pre, x.dPreTot, sizeof(pre), "prefix tot copy");
  if (n_out) *n_out = tot[2];
  if (arena_len) *arena_len = pre;
  // a batch over the wire capacities wrote nothing (see lkf_output_device); the
  // prefix arena never needs more than the wire arena
  if (tot[2] > e->cfg.max_out_pkts || tot[3] > e->cfg.max_out_bytes || pre > e->cfg.max_out_bytes) {
    e->err = "output or tuple capacity exceeded";
    return LKF_ENOSPC;
  }
  return LKF_OK;
}
static int prefix_copy(lkf_engine *e, BatchCtx &x, lkf_pre *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap,
                       uint64_t *n_out, uint64_t *arena_len) {
  uint64_t n = 0, len = 0;
  const int rc = prefix_totals(e, x, &n, &len);
  if (n_out) *n_out = n;
  if (arena_len) *arena_len = len;
  if (rc) return rc;
  if (n > cap || len > arena_cap) return LKF_ENOSPC;
  if (out && n) {
    const int r = copy_to_host(e, out, x.dPre, n * sizeof(lkf_pre), "drain prefix recs");
    if (r) return r;
  }
  if (arena && len) return copy_to_host(e, arena, x.dOutArena, len, "drain prefix bytes");
  return LKF_OK;
}

int lkf_output_prefix_device(lkf_engine *e, const lkf_pre **d_out, uint64_t *n_out, const uint8_t **d_arena,
                             uint64_t *arena_len) {
  if (!e) return LKF_EINVAL;
  int rc = lkf_sync(e);
  if (rc) return rc;
  if (n_out) *n_out = 0;
  if (arena_len) *arena_len = 0;
  if (e->lastCtx < 0) {
    if (d_out) *d_out = e->ctx[0].dPre;
    if (d_arena) *d_arena = e->ctx[0].dOutArena;
    return LKF_OK;
  }
  BatchCtx &x = e->ctx[e->lastCtx];
  rc = prefix_totals(e, x, n_out, arena_len);
  if (rc) return rc;
  if (d_out) *d_out = x.dPre;
  if (d_arena) *d_arena = x.dOutArena;
  return LKF_OK;
}

int lkf_drain_prefix(lkf_engine *e, lkf_pre *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap, uint64_t *n_out,
                     uint64_t *arena_len) {
  if (!e) return LKF_EINVAL;
  const int rc = lkf_sync(e);
  if (rc) return rc;
  if (e->lastCtx < 0) {
    if (n_out) *n_out = 0;
    if (arena_len) *arena_len = 0;
    return LKF_OK;
  }
  return prefix_copy(e, e->ctx[e->lastCtx], out, cap, arena, arena_cap, n_out, arena_len);
}

int lkf_drain_prefix_run(lkf_engine *e, uint32_t age, lkf_pre *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap,
                         uint64_t *n_out, uint64_t *arena_len) {
  if (!e || age >= uint32_t(lkf_engine::kCtx) || uint64_t(age) >= e->nRuns) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[(e->nRuns - 1 - age) % lkf_engine::kCtx];
  if (const int rc = egress_is(e, x, LKF_EGRESS_PREFIX)) return rc;
  HIPCHK(hipEventSynchronize(x.emitted), "wait emitted");
  return prefix_copy(e, x, out, cap, arena, arena_cap, n_out, arena_len);
}

int lkf_output_device(lkf_engine *e, const lkf_out **d_out, uint64_t *n_out, const uint8_t **d_arena,
                      uint64_t *arena_len) {
  if (!e) return LKF_EINVAL;
  int rc = lkf_sync(e);
  if (rc) return rc;
  if (e->lastCtx < 0) {
    if (d_out) *d_out = e->ctx[0].dOut;
    if (d_arena) *d_arena = e->ctx[0].dOutArena;
    if (n_out) *n_out = 0;
    if (arena_len) *arena_len = 0;
    return LKF_OK;
  }
  BatchCtx &x = e->ctx[e->lastCtx];
  rc = egress_is(e, x, LKF_EGRESS_WIRE);
  if (rc) return rc;
  uint64_t tot[4];
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  // a batch whose output exceeded the engine's capacity wrote nothing (k_emit
  // flags it; lkf_sync reported it once): never hand out a range beyond the
  // output buffers, whatever the caller did with that report
  if (tot[2] > e->cfg.max_out_pkts || tot[3] > e->cfg.max_out_bytes) {
    e->err = "output or tuple capacity exceeded";
    return LKF_ENOSPC;
  }
  if (d_out) *d_out = x.dOut;
  if (d_arena) *d_arena = x.dOutArena;
  if (n_out) *n_out = tot[2];
  if (arena_len) *arena_len = tot[3];
  return LKF_OK;
}

int lkf_drain(lkf_engine *e, lkf_out *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap, uint64_t *n_out,
              uint64_t *arena_len) {
  const lkf_out *dOut = nullptr;
  const uint8_t *dAr = nullptr;
  uint64_t n = 0, len = 0;
  int rc = lkf_output_device(e, &dOut, &n, &dAr, &len);
  if (rc) return rc;
  if (n_out) *n_out = n;
  if (arena_len) *arena_len = len;
  if (n > cap || len > arena_cap) return LKF_ENOSPC;
  if (out && n) {
    const int r = copy_to_host(e, out, dOut, n * sizeof(lkf_out), "drain recs");
    if (r) return r;
  }
  if (arena && len) return copy_to_host(e, arena, dAr, len, "drain bytes");
  return LKF_OK;
}

int lkf_drain_run(lkf_engine *e, uint32_t age, lkf_out *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap,
                  uint64_t *n_out, uint64_t *arena_len) {
  if (!e || age >= uint32_t(lkf_engine::kCtx) || uint64_t(age) >= e->nRuns) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[(e->nRuns - 1 - age) % lkf_engine::kCtx];
  if (const int rc = egress_is(e, x, LKF_EGRESS_WIRE)) return rc;
  HIPCHK(hipEventSynchronize(x.emitted), "wait emitted");
  uint64_t tot[4];
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  if (n_out) *n_out = tot[2];
  if (arena_len) *arena_len = tot[3];
  if (tot[2] > e->cfg.max_out_pkts || tot[3] > e->cfg.max_out_bytes) {  // (see lkf_output_device)
    e->err = "output or tuple capacity exceeded";
    return LKF_ENOSPC;
  }
  if (tot[2] > cap || tot[3] > arena_cap) return LKF_ENOSPC;
  if (out && tot[2]) {
    const int r = copy_to_host(e, out, x.dOut, tot[2] * sizeof(lkf_out), "drain recs");
    if (r) return r;
  }
  if (arena && tot[3]) {
    const int r = copy_to_host(e, arena, x.dOutArena, tot[3], "drain bytes");
    if (r) return r;
  }
  return LKF_OK;
}

int lkf_drain_run_async(lkf_engine *e, uint32_t age, lkf_out *out, uint64_t cap, uint8_t *arena, uint64_t arena_cap,
                        uint64_t *n_out, uint64_t *arena_len) {
  if (!e || age >= uint32_t(lkf_engine::kCtx) || uint64_t(age) >= e->nRuns) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (!e->d2hS) HIPCHK(hipStreamCreateWithFlags(e->d2hS.put(), hipStreamNonBlocking), "copy stream");
  BatchCtx &x = e->ctx[(e->nRuns - 1 - age) % lkf_engine::kCtx];
  if (const int rc = egress_is(e, x, LKF_EGRESS_WIRE)) return rc;
  HIPCHK(hipEventSynchronize(x.emitted), "wait emitted");
  uint64_t tot[4];
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  if (n_out) *n_out = tot[2];
  if (arena_len) *arena_len = tot[3];
  if (tot[2] > e->cfg.max_out_pkts || tot[3] > e->cfg.max_out_bytes) {  // (see lkf_output_device)
    e->err = "output or tuple capacity exceeded";
    return LKF_ENOSPC;
  }
  if (tot[2] > cap || tot[3] > arena_cap) return LKF_ENOSPC;
  // (the context is reused only after run n + 3 is enqueued, which the caller
  // does after lkf_drain_wait: the source stays valid while the copies run)
  if (out && tot[2]) {
    CHKRANGE(x.dOut, tot[2] * sizeof(lkf_out), "async d2h");
    HIPCHK(hipMemcpyAsync(out, x.dOut, tot[2] * sizeof(lkf_out), hipMemcpyDeviceToHost, e->d2hS), "drain recs");
  }
  if (arena && tot[3]) {
    CHKRANGE(x.dOutArena, tot[3], "async d2h");
    HIPCHK(hipMemcpyAsync(arena, x.dOutArena, tot[3], hipMemcpyDeviceToHost, e->d2hS), "drain bytes");
  }
  return LKF_OK;
}

int lkf_drain_wait(lkf_engine *e) {
  if (!e) return LKF_EINVAL;
  if (e->d2hS) HIPCHK(hipStreamSynchronize(e->d2hS), "copy stream sync");
  return LKF_OK;
}

// ---- SRTP protect ---------------------------------------------------------
static int srtp_init(lkf_engine *e) {
  if (e->dAesTab) return LKF_OK;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(e->dAesTab.alloc(256 + 64), "alloc aes tables");
  HIPCHK(e->dSrtpDT.alloc(e->cfg.max_downtracks), "alloc srtp dt");
  HIPCHK(hipMemsetAsync(e->dSrtpDT, 0, sizeof(SrtpDT) * e->cfg.max_downtracks, e->own), "srtp dt init");
  HIPCHK(launch_aes_tables(e->own, e->dAesTab), "aes tables");
  HIPCHK(hipStreamSynchronize(e->own), "srtp init sync");
  for (auto &r : e->protRing)
    for (auto &ev : r) HIPCHK(ev.create(true), "protect event");
  e->protRun.assign(256, 0);
  return LKF_OK;
}

int32_t lkf_add_transport(lkf_engine *e, const lkf_transport_params *p) {
  if (!e || !p || (p->profile != LKF_SRTP_AES128_CM_HMAC_SHA1_80 && p->profile != LKF_SRTP_AEAD_AES_128_GCM))
    return LKF_EINVAL;
  int rc = srtp_init(e);
  if (rc) return rc;
  const uint32_t t = uint32_t(e->transports.size());
  if (t + 1 > e->dTransports.cap()) {  // grow, keeping the old ones; queued protect stages read the keys
    rc = drain_streams(e);
    if (rc) return rc;
    const uint32_t cap = std::max<uint32_t>(64, 2 * uint32_t(e->dTransports.cap()));
    DevBuf<lkf_transport_params> np;
    DevBuf<SrtpKeys> nk;
    HIPCHK(np.alloc(cap), "alloc transports");
    HIPCHK(nk.alloc(cap), "alloc srtp keys");
    if (t) {
      HIPCHK(hipMemcpy(np, e->dTransports, t * sizeof(lkf_transport_params), hipMemcpyDeviceToDevice),
             "copy transports");
      HIPCHK(hipMemcpy(nk, e->dSrtpKeys, t * sizeof(SrtpKeys), hipMemcpyDeviceToDevice), "copy keys");
    }
    // the SRTCP keys, slot tables and ranges (the tables of new handles start empty)
    DevBuf<SrtpKeys> nck;
    DevBuf<lkf_transport_srtcp> nrx, nspec;
    DevBuf<uint32_t> nrange;
    HIPCHK(nck.alloc(cap), "alloc srtcp keys");
    HIPCHK(nrx.alloc(cap), "alloc srtcp rx state");
    HIPCHK(nspec.alloc(cap), "alloc srtcp rx spec state");
    HIPCHK(nrange.alloc(2 * size_t(cap)), "alloc srtcp ranges");
    HIPCHK(hipMemset(nrx, 0, cap * sizeof(lkf_transport_srtcp)), "srtcp rx init");
    if (t) {
      HIPCHK(hipMemcpy(nck, e->dSrtcpKeys, t * sizeof(SrtpKeys), hipMemcpyDeviceToDevice), "copy srtcp keys");
      HIPCHK(hipMemcpy(nrx, e->dSrtcpRx, t * sizeof(lkf_transport_srtcp), hipMemcpyDeviceToDevice),
             "copy srtcp rx state");
    }
    rc = upload_done(e);  // (the sender stream does not order against these)
    if (rc) return rc;
    e->dTransports = std::move(np);
    e->dSrtpKeys = std::move(nk);
    e->dSrtcpKeys = std::move(nck);
    e->dSrtcpRx = std::move(nrx);
    e->dSrtcpRxSpec = std::move(nspec);
    e->dSrtcpRange = std::move(nrange);
  }
  e->transports.push_back(*p);
  HIPCHK(hipMemcpyAsync(e->dTransports + t, &e->transports.back(), sizeof(*p), hipMemcpyHostToDevice, e->own),
         "transport copy");
  HIPCHK(launch_srtp_keys(e->own, e->dTransports + t, t, 1, e->dAesTab, e->dSrtpKeys, 0), "srtp keys");
  HIPCHK(launch_srtp_keys(e->own, e->dTransports + t, t, 1, e->dAesTab, e->dSrtcpKeys, 3), "srtcp keys");
  HIPCHK(hipStreamSynchronize(e->own), "srtp keys sync");
  return int32_t(t);
}

int lkf_set_downtrack_transport(lkf_engine *e, int32_t dt, int32_t t) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size()) || t < -1 || t >= int32_t(e->transports.size()))
    return LKF_EINVAL;
  int rc = srtp_init(e);
  if (rc) return rc;
  rc = flush_topology(e);  // (the DownTrack's static parameters are on the device)
  if (rc) return rc;
  rc = drain_streams(e);  // queued protect stages read the binding
  if (rc) return rc;
  SrtpDT v{uint32_t(t + 1), 0, 0};
  HIPCHK(hipMemcpy(e->dSrtpDT + dt, &v, sizeof(v), hipMemcpyHostToDevice), "srtp bind");
  // its transport-wide sequence numbers: the transport's counter from now on
  e->dtTransport[size_t(dt)] = t;
  const uint32_t grp = t >= 0 ? (0x80000000u | uint32_t(t)) : uint32_t(dt);
  HIPCHK(hipMemcpy(reinterpret_cast<uint8_t *>(e->dDTs + dt) + offsetof(DevDT, twccGroup), &grp, sizeof(grp),
                   hipMemcpyHostToDevice),
         "twcc group");
  if (e->dtp[size_t(dt)].ext_transport_cc) e->twccDirty = true;
  return upload_done(e);
}

// Host bookkeeping alone: the next demux call rebuilds the routing table.
int lkf_set_downtrack_rtcp_transport(lkf_engine *e, int32_t dt, int32_t t) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size()) || t < -1 || t >= int32_t(e->transports.size()))
    return LKF_EINVAL;
  e->dtRtcpTransport[size_t(dt)] = t;
  e->dmxDirty = true;
  return LKF_OK;
}

// pion/rtp NewAbsSendTimeExtension(t).Marshal(): NTP time >> 14, 24 bits
static uint32_t abs_send_time(int64_t unixNs) {
  const uint64_t u = uint64_t(unixNs);
  const uint64_t sec = u / 1000000000ull + 0x83AA7E80ull;
  const uint64_t frac = ((u % 1000000000ull) << 32) / 1000000000ull;
  return uint32_t((((sec << 32) | frac) >> 14) & 0xFFFFFF);
}

int lkf_protect(lkf_engine *e, int64_t send_time_ns) {
  if (!e || e->lastCtx < 0) return LKF_EINVAL;
  int rc = srtp_init(e);
  if (rc) return rc;
  BatchCtx &x = e->ctx[e->lastCtx];
  rc = egress_is(e, x, LKF_EGRESS_WIRE);  // (no SRTP over prefixes: that host protects in pion)
  if (rc) return rc;
  if (!x.dProt)
    HIPCHK(x.dProt.alloc(e->cfg.max_out_bytes + 16 * uint64_t(e->cfg.max_out_pkts)), "alloc protected arena");
  SrtpProtectArgs a;
  a.tab = e->dAesTab;
  a.totals = x.dTot + 2;
  a.out = x.dOut;
  a.arena = x.dOutArena;
  a.prot = x.dProt;
  a.dts = e->dDTs;
  a.sd = e->dSrtpDT;
  a.keys = e->dSrtpKeys;
  a.cap = e->cfg.max_out_pkts;
  a.absVal = abs_send_time(send_time_ns);
  // after the run's emit stage on the emit stream; the context's "emitted"
  // event (what its next reuse waits for) moves behind the protect stage
  const size_t slot = (e->nRuns - 1) % 256;
  HIPCHK(hipEventRecord(e->protRing[slot][0], e->emitS), "event");
  HIPCHK(launch_srtp_protect(e->emitS, a, uint32_t(e->dtp.size()), e->dPerm, x.dRecBase, x.dFwdCnt), "protect");
  HIPCHK(hipEventRecord(e->protRing[slot][1], e->emitS), "event");
  HIPCHK(hipEventRecord(x.emitted, e->emitS), "event");
  e->protRun[slot] = 1;
  x.protectedRun = true;
  return LKF_OK;
}

int lkf_output_protected_device(lkf_engine *e, const uint8_t **d_arena, uint64_t *arena_len) {
  if (!e || e->lastCtx < 0) return LKF_EINVAL;
  int rc = lkf_sync(e);
  if (rc) return rc;
  BatchCtx &x = e->ctx[e->lastCtx];
  if (!x.protectedRun) {
    e->err = "the last run was not protected (lkf_protect)";
    return LKF_EINVAL;
  }
  uint64_t tot[4];
  D2H(tot, x.dTot, sizeof(tot), "tot copy");
  if (d_arena) *d_arena = x.dProt;
  if (arena_len) *arena_len = tot[3] + 16 * tot[2];
  return LKF_OK;
}

int lkf_protect_timing_window(lkf_engine *e, uint32_t n, float *protect_ms) {
  if (!e || !e->dAesTab || n == 0 || n > 256 || n > e->nRuns) return LKF_EINVAL;
  float sum = 0;
  for (uint64_t r = e->nRuns - n; r < e->nRuns; r++) {
    if (!e->protRun[r % 256]) return LKF_EINVAL;
    HIPCHK(hipEventSynchronize(e->protRing[r % 256][1]), "evsync");
    float a = 0;
    HIPCHK(hipEventElapsedTime(&a, e->protRing[r % 256][0], e->protRing[r % 256][1]), "elapsed");
    sum += a;
  }
  if (protect_ms) *protect_ms = sum;
  return LKF_OK;
}

int lkf_drain_protected(lkf_engine *e, uint8_t *arena, uint64_t cap, uint64_t *arena_len) {
  const uint8_t *d = nullptr;
  uint64_t len = 0;
  int rc = lkf_output_protected_device(e, &d, &len);
  if (rc) return rc;
  if (arena_len) *arena_len = len;
  if (len > cap) return LKF_ENOSPC;
  if (arena && len) D2H(arena, d, len, "drain protected");
  return LKF_OK;
}

int lkf_sender_stats_get(lkf_engine *e, int32_t dt, lkf_sender_stats *out) {
  if (!e || !out || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  SenderStats s;
  D2H(&s, e->dSS + dt, sizeof(s), "sender stats copy");
  std::memset(out, 0, sizeof(*out));
  out->ext_start_sn = s.extStartSN;
  out->ext_highest_sn = s.extHighestSN;
  out->ext_start_ts = s.extStartTS;
  out->ext_highest_ts = s.extHighestTS;
  out->first_time_ns = s.firstTime;
  out->highest_time_ns = s.highestTime;
  out->last_transit = s.lastTransit;
  out->last_jitter_ext_ts = s.lastJitterExtTimestamp;
  out->bytes = s.bytes;
  out->header_bytes = s.headerBytes;
  out->bytes_duplicate = s.bytesDuplicate;
  out->header_bytes_duplicate = s.headerBytesDuplicate;
  out->bytes_padding = s.bytesPadding;
  out->header_bytes_padding = s.headerBytesPadding;
  out->packets_duplicate = s.packetsDuplicate;
  out->packets_padding = s.packetsPadding;
  out->packets_out_of_order = s.packetsOutOfOrder;
  out->packets_lost = s.packetsLost;
  out->jitter = s.jitter;
  out->max_jitter = s.maxJitter;
  out->frames = s.frames;
  out->key_frames = s.keyFrames;
  out->initialized = s.initialized;
  out->clock_rate = s.clockRate;
  D2H(out->gap_histogram, e->dSSGap + size_t(dt) * kGapWords, kGapBins * sizeof(uint32_t), "sender gap copy");
  return LKF_OK;
}

int lkf_sender_sninfo(lkf_engine *e, int32_t dt, uint64_t esn, uint32_t *out) {
  if (!e || !out || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  D2H(out, e->dSSRing + size_t(dt) * kSnInfoSize + (esn & (kSnInfoSize - 1)), sizeof(uint32_t), "sninfo copy");
  return LKF_OK;
}

int lkf_sender_stats_seed(lkf_engine *e, int32_t dt, int32_t from_dt) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size()) || from_dt < 0 || from_dt >= int32_t(e->dtp.size()))
    return LKF_EINVAL;
  STEP(quiesce(e));
  SenderStats from, to;
  D2H(&from, e->dSS + from_dt, sizeof(from), "sender stats copy");
  if (!from.initialized) return LKF_OK;  // rtpStatsBase.seed: from must be initialized
  D2H(&to, e->dSS + dt, sizeof(to), "sender stats copy");
  from.clockRate = to.clockRate;  // params are not seeded
  HIPCHK(hipMemcpy(e->dSS + dt, &from, sizeof(from), hipMemcpyHostToDevice), "sender stats seed");
  HIPCHK(hipMemcpy(e->dSSGap + size_t(dt) * kGapWords, e->dSSGap + size_t(from_dt) * kGapWords,
                   kGapWords * sizeof(uint32_t), hipMemcpyDeviceToDevice),
         "sender gap seed");
  HIPCHK(hipMemcpy(e->dSSRing + size_t(dt) * kSnInfoSize, e->dSSRing + size_t(from_dt) * kSnInfoSize,
                   kSnInfoSize * sizeof(uint32_t), hipMemcpyDeviceToDevice),
         "sender ring seed");
  {  // the RTCP half: what rtpStatsBase.seed (rtpstats_base.go:206-279) and RTPStatsSender.Seed copy of it;
     // endTime is not cloned, the three log counters are not part of Seed
    SenderRtcp rf, rt;
    D2H(&rf, e->dRtcp + from_dt, sizeof(rf), "sender rtcp copy");
    D2H(&rt, e->dRtcp + dt, sizeof(rt), "sender rtcp copy");
    rf.endTime = rt.endTime;
    rf.clockSkewCount = rt.clockSkewCount;
    rf.outOfOrderSenderReportCount = rt.outOfOrderSenderReportCount;
    rf.metadataCacheOverflowCount = rt.metadataCacheOverflowCount;
    HIPCHK(hipMemcpy(e->dRtcp + dt, &rf, sizeof(rf), hipMemcpyHostToDevice), "sender rtcp seed");
  }
  return upload_done(e);
}

// ---- the DownTrack RTCP loop (rtcp_kernels.hip) -------------------------------
static_assert(sizeof(lkf_sender_rtcp) == sizeof(SenderRtcp), "lkf_sender_rtcp is SenderRtcp's layout");
static_assert(offsetof(lkf_sender_rtcp, snapshot) == offsetof(SenderRtcp, snap) &&
                  offsetof(lkf_sender_rtcp, sr_first) == offsetof(SenderRtcp, srFirst) &&
                  offsetof(lkf_sender_rtcp, end_time_ns) == offsetof(SenderRtcp, endTime) &&
                  offsetof(lkf_sender_snapshot, interval_stats) == offsetof(RtcpSnapshot, intervalStats),
              "lkf_sender_rtcp is SenderRtcp's layout");
static_assert(sizeof(lkf_rtcp_fb) == 48 && sizeof(lkf_rtcp_sr) == 40 && sizeof(lkf_rtp_delta_info) == 120 &&
                  sizeof(lkf_rtcp_fb_result) == 8 && sizeof(lkf_rtcp_sr_req) == 8,
              "RTCP call records");

int lkf_sender_rtcp_get(lkf_engine *e, int32_t dt, lkf_sender_rtcp *out) {
  if (!e || !out || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  D2H(out, e->dRtcp + dt, sizeof(*out), "sender rtcp copy");
  return LKF_OK;
}

// The three calls run behind the sender stream's queued work (Order::BehindSender):
// the input goes up, the kernel runs and the results come back on that stream.
// Their scratch is one family: input bytes, group bounds, result bytes.
static int rtcp_grow(Frame &f, size_t inBytes, size_t groups, size_t outBytes) {
  lkf_engine *e = f.e;
  return f.grow("alloc rtcp scratch", want(e->dRtcpIn, inBytes, 1 << 16, 2 * inBytes),
                want(e->dRtcpGroups, groups, 4096, 2 * groups), want(e->dRtcpOut, outBytes, 1 << 16, 2 * outBytes));
}

int lkf_rtcp_feedback(lkf_engine *e, const lkf_rtcp_fb *in, uint32_t n, int64_t now_ns, lkf_rtcp_fb_result *out) {
  if (!e || (n && (!in || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  // groups: one per DownTrack's contiguous entries (a DownTrack must not reappear)
  std::vector<uint32_t> g;
  STEP(check_handles(&in[0].dt, sizeof(*in), n, e->dtp.size(), {Repeat::Groups, &g, true}));
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  STEP(rtcp_grow(f, size_t(n) * sizeof(lkf_rtcp_fb), g.size(), size_t(n) * sizeof(lkf_rtcp_fb_result)));
  STEP(f.up(e->dRtcpIn, in, size_t(n) * sizeof(lkf_rtcp_fb), "rtcp fb copy"));
  STEP(f.up(e->dRtcpGroups, g.data(), g.size() * sizeof(uint32_t), "rtcp groups copy"));
  RrUpdateLaunch a;
  a.in = reinterpret_cast<const lkf_rtcp_fb *>(e->dRtcpIn.get());
  a.gBegin = e->dRtcpGroups;
  a.ngroups = uint32_t(g.size() - 1);
  a.n = n;
  a.now = now_ns;
  a.ss = e->dSS;
  a.ring = e->dSSRing;
  a.rtcp = e->dRtcp;
  a.ndts = uint32_t(e->dtp.size());
  a.out = reinterpret_cast<lkf_rtcp_fb_result *>(e->dRtcpOut.get());
  HIPCHK(launch_rr_update(f.s, a), "rr update");
  STEP(f.down(out, e->dRtcpOut, size_t(n) * sizeof(lkf_rtcp_fb_result), "rtcp results copy"));
  return f.wait();
}

int lkf_rtcp_sender_reports(lkf_engine *e, const lkf_rtcp_sr_req *req, uint32_t n, int64_t now_ns, lkf_rtcp_sr *out,
                            uint8_t *wire28) {
  if (!e || (n && (!req || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  // one thread per request: a DownTrack's state has one writer
  STEP(check_handles(&req[0].dt, sizeof(*req), n, e->dtp.size(), {Repeat::DistinctEorder}));
  // results: n records (40 B each, so the wire bytes behind them stay 4-B aligned), then 28 B per request
  const size_t recBytes = size_t(n) * sizeof(lkf_rtcp_sr), wireBytes = wire28 ? size_t(n) * 28 : 0;
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  STEP(rtcp_grow(f, size_t(n) * sizeof(lkf_rtcp_sr_req), 0, recBytes + wireBytes));
  STEP(f.up(e->dRtcpIn, req, size_t(n) * sizeof(lkf_rtcp_sr_req), "rtcp sr requests copy"));
  SrBuildLaunch a;
  a.req = reinterpret_cast<const lkf_rtcp_sr_req *>(e->dRtcpIn.get());
  a.n = n;
  a.now = now_ns;
  a.ss = e->dSS;
  a.rtcp = e->dRtcp;
  a.dts = e->dDTs;
  a.ndts = uint32_t(e->dtp.size());
  a.out = reinterpret_cast<lkf_rtcp_sr *>(e->dRtcpOut.get());
  a.wire = wire28 ? e->dRtcpOut.get() + recBytes : nullptr;
  HIPCHK(launch_sr_build(f.s, a), "sr build");
  STEP(f.down(out, e->dRtcpOut, recBytes, "rtcp results copy"));
  STEP(f.wait());
  if (wire28) D2H(wire28, e->dRtcpOut.get() + recBytes, wireBytes, "rtcp wire copy");
  return LKF_OK;
}

int lkf_sender_delta_info(lkf_engine *e, const int32_t *dts, uint32_t n, lkf_rtp_delta_info *out) {
  if (!e || (n && (!dts || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  STEP(check_handles(dts, sizeof(*dts), n, e->dtp.size(), {Repeat::DistinctEorder}));
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  STEP(rtcp_grow(f, size_t(n) * sizeof(int32_t), 0, size_t(n) * sizeof(lkf_rtp_delta_info)));
  STEP(f.up(e->dRtcpIn, dts, size_t(n) * sizeof(int32_t), "rtcp dts copy"));
  DeltaSenderLaunch a;
  a.dts = reinterpret_cast<const int32_t *>(e->dRtcpIn.get());
  a.n = n;
  a.ss = e->dSS;
  a.rtcp = e->dRtcp;
  a.ndts = uint32_t(e->dtp.size());
  a.out = reinterpret_cast<lkf_rtp_delta_info *>(e->dRtcpOut.get());
  HIPCHK(launch_delta_sender(f.s, a), "delta sender");
  STEP(f.down(out, e->dRtcpOut, size_t(n) * sizeof(lkf_rtp_delta_info), "rtcp results copy"));
  return f.wait();
}

int lkf_get_state(lkf_engine *e, int32_t dt, lkf_fwd_state *o) {
  if (!e || !o || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  DTHot h;
  D2H(&h, e->dHot + dt, sizeof(h), "state copy");
  std::memset(o, 0, sizeof(*o));
  if (!(h.flags & F_STARTED)) return LKF_OK;  // GetState forwarder.go:344-346
  o->started = 1;
  o->reference_layer_spatial = h.referenceLayerSpatial;
  o->pre_start_time_ns = h.preStartTime;
  o->ext_first_ts = h.extFirstTS;
  o->ref_ts_offset = h.refTSOffset;
  o->ext_last_sn = h.extLastSN;
  o->ext_second_last_sn = h.extSecondLastSN;
  o->ext_last_ts = h.extLastTS;
  o->ext_second_last_ts = h.extSecondLastTS;
  o->last_marker = (h.flags & F_LAST_MARKER) ? 1 : 0;
  o->second_last_marker = (h.flags & F_SECOND_LAST_MARKER) ? 1 : 0;
  o->has_vp8 = (h.flags & F_VP8) ? 1 : 0;
  o->vp8_ext_last_picture_id = h.extLastPictureId;
  o->vp8_picture_id_used = (h.flags & F_PICID_USED) ? 1 : 0;
  o->vp8_last_tl0picidx = h.lastTl0;
  o->vp8_tl0picidx_used = (h.flags & F_TL0_USED) ? 1 : 0;
  o->vp8_tid_used = (h.flags & F_TID_USED) ? 1 : 0;
  o->vp8_last_keyidx = h.lastKeyIdx;
  o->vp8_keyidx_used = (h.flags & F_KEYIDX_USED) ? 1 : 0;
  return LKF_OK;
}

int lkf_seed_state(lkf_engine *e, int32_t dt, const lkf_fwd_state *i) {
  if (!e || !i || dt < 0 || dt >= int32_t(e->dtp.size())) return LKF_EINVAL;
  if (!i->started) return LKF_OK;  // SeedState forwarder.go:360-362
  STEP(quiesce(e));
  DTHot h;
  D2H(&h, e->dHot + dt, sizeof(h), "state copy");
  auto setf = [&](uint32_t f, bool v) { h.flags = v ? (h.flags | f) : (h.flags & ~f); };
  // RTPMunger.SeedLast rtpmunger.go:126-133
  h.extLastSN = i->ext_last_sn;
  h.extSecondLastSN = i->ext_second_last_sn;
  h.extLastTS = i->ext_last_ts;
  h.extSecondLastTS = i->ext_second_last_ts;
  setf(F_LAST_MARKER, i->last_marker);
  setf(F_SECOND_LAST_MARKER, i->second_last_marker);
  // codecMunger.SeedState vp8.go:99-109 (only a VP8 munger takes VP8State)
  if ((h.flags & F_VP8) && i->has_vp8) {
    h.extLastPictureId = i->vp8_ext_last_picture_id;
    setf(F_PICID_USED, i->vp8_picture_id_used);
    h.lastTl0 = i->vp8_last_tl0picidx;
    setf(F_TL0_USED, i->vp8_tl0picidx_used);
    setf(F_TID_USED, i->vp8_tid_used);
    h.lastKeyIdx = i->vp8_last_keyidx;
    setf(F_KEYIDX_USED, i->vp8_keyidx_used);
  }
  setf(F_STARTED, true);
  h.referenceLayerSpatial = i->reference_layer_spatial;
  h.preStartTime = i->pre_start_time_ns;
  h.extFirstTS = i->ext_first_ts;
  h.refTSOffset = i->ref_ts_offset;
  return write_row(e, e->dHot + dt, h, "seed copy");
}

int lkf_seq_lookup(lkf_engine *e, int32_t dt, const uint16_t *sns, uint32_t n, int64_t now_ns, lkf_seq_meta *out,
                   uint32_t *n_out) {
  if (!e || dt < 0 || dt >= int32_t(e->dtp.size()) || (n && (!sns || !out))) return LKF_EINVAL;
  Frame f(e, Order::Quiesced);
  STEP(f.open());
  STEP(f.grow("alloc seq lookup scratch", want(e->dSns, n, 256), want(e->dSeqOut, n, 256)));
  if (!e->dSeqN) HIPCHK(e->dSeqN.alloc(1), "alloc");
  if (n) STEP(f.up(e->dSns, sns, n * sizeof(uint16_t), "sns copy"));
  STEP(f.uploaded());
  HIPCHK(launch_seq_lookup(f.s, e->dHot, e->dSeq, e->cfg.seq_size, e->dSrm, e->srmStride, e->srmCap, uint32_t(dt),
                           e->dSns, n, now_ns / 1000000,
                           e->dSeqOut, e->dSeqN),
         "seq lookup");
  STEP(f.wait());
  uint32_t cnt = 0;
  D2H(&cnt, e->dSeqN, sizeof(cnt), "n copy");
  if (cnt) D2H(out, e->dSeqOut, cnt * sizeof(lkf_seq_meta), "out copy");
  if (n_out) *n_out = cnt;
  return LKF_OK;
}

// The seven NACK -> RTX buffers grow together, dRtxOff last: its capacity is
// what all of them hold (0 after a failed grow, which the next call retries).
static int rtx_grow(Frame &f, uint32_t n) {
  lkf_engine *e = f.e;
  return f.grow("alloc rtx scratch", want(e->dNacks, n, 1024), want(e->dNackG, uint64_t(n) + 1, 1025),
                want(e->dNackValid, n, 1024), want(e->dRtx, n, 1024), want(e->dRtxSrc, n, 1024),
                want(e->dRtxLen, n, 1024), want(e->dRtxOff, n, 1024));
}

// The lookup itself on the frame's stream: m NACKs at `list` in ngroups non-empty
// DownTrack groups (bounds in dNackG), the records compacted on the host.
static int rtx_lookup_run(Frame &f, const lkf_nack *list, uint32_t ngroups, uint32_t m, int64_t now_ns, lkf_rtx *out,
                          uint32_t cap, uint32_t *n_out) {
  lkf_engine *e = f.e;
  HIPCHK(launch_rtx_lookup(f.s, e->dHot, e->dSeq, e->cfg.seq_size, e->dSrm, e->srmStride, e->srmCap, list, e->dNackG,
                           ngroups, now_ns / 1000000, e->dRtx, e->dNackValid),
         "rtx lookup");
  std::vector<lkf_rtx> r(m);
  std::vector<uint32_t> v(m);
  STEP(f.down(r.data(), e->dRtx, m * sizeof(lkf_rtx), "rtx copy"));
  STEP(f.down(v.data(), e->dNackValid, m * sizeof(uint32_t), "valid copy"));
  STEP(f.wait());
  uint32_t k = 0;
  for (uint32_t i = 0; i < m; i++) k += v[i];
  *n_out = k;
  if (cap < k) return LKF_ENOSPC;
  k = 0;
  for (uint32_t i = 0; i < m; i++)
    if (v[i]) out[k++] = r[i];
  return LKF_OK;
}

int lkf_rtx_lookup(lkf_engine *e, const lkf_nack *nacks, uint32_t n, int64_t now_ns, lkf_rtx *out, uint32_t cap,
                   uint32_t *n_out) {
  if (!e || !n_out || (n && !nacks)) return LKF_EINVAL;
  *n_out = 0;
  // groups: one per DownTrack's contiguous NACK list (a DownTrack must not reappear)
  std::vector<uint32_t> gStart;
  if (n)  // (a removed DownTrack answers no NACK: its group is left out)
    STEP(check_handles(&nacks[0].dt, sizeof(*nacks), n, e->dtp.size(),
                       {Repeat::Groups, &gStart, false, e->active.data(), Inactive::Skip}));
  e->rtxNow = now_ns;  // retransmitPackets' time.Now() for the RTX sendingPacket (lkf_rtx_emit)
  if (gStart.empty()) return LKF_OK;
  // group ends: the next group's start or the end of its DownTrack's run
  std::vector<uint32_t> gb(gStart.size() + 1);
  std::vector<lkf_nack> packed;
  packed.reserve(n);
  for (size_t g = 0; g < gStart.size(); g++) {
    gb[g] = uint32_t(packed.size());
    uint32_t i = gStart[g];
    const int32_t dt = nacks[i].dt;
    while (i < n && nacks[i].dt == dt) packed.push_back(nacks[i++]);
  }
  gb[gStart.size()] = uint32_t(packed.size());
  const uint32_t m = uint32_t(packed.size());
  // The lookup reads and updates the sequencer records and the DownTracks'
  // hot state, which between runs only the decide stream touches: ordered on
  // that stream behind the queued decides (their emits keep running), as the
  // allocation calls.  (The decide stream is waited for only if the scratch regrows.)
  Frame f(e, Order::BehindDecide);
  STEP(f.open());
  STEP(rtx_grow(f, m));
  STEP(f.up(e->dNacks, packed.data(), m * sizeof(lkf_nack), "nacks copy"));
  STEP(f.up(e->dNackG, gb.data(), gb.size() * sizeof(uint32_t), "groups copy"));
  return rtx_lookup_run(f, e->dNacks, uint32_t(gStart.size()), m, now_ns, out, cap, n_out);
}

// ---- RTCP ingress (rtcp_kernels.hip k_rtcp_in_*; the parse is rtcp_in_device.h) ----
static_assert(sizeof(lkf_rtcp_raw) == 12 && sizeof(lkf_rtcp_in_result) == 48 && sizeof(lkf_rtcp_ref) == 16,
              "RTCP ingress records");

// The call frame is the three RTCP calls' (Order::BehindSender): the sender
// stream ordered after every queued stage, the buffers grown only while it is idle.
// Count pass -> scans -> the totals back on the host (the lists are sized by
// them, never by a guess about the bytes) -> write pass -> k_rr_update on the
// device-resident fb list -> the fold of its results into the entries.
// `arena`: the compound packets in host memory, uploaded first; NULL: they are
// the arena_len bytes at dArena already (lkf_rtcp_ingest_unprotected).
static int rtcp_ingest_run(lkf_engine *e, const lkf_rtcp_raw *in, uint32_t n, const uint8_t *arena,
                           const uint8_t *dArena, uint64_t arena_len, int64_t now_ns, lkf_rtcp_in_result *out,
                           lkf_rtcp_fb *fb, lkf_rtcp_fb_result *fb_out, uint32_t fb_cap, uint32_t *n_fb,
                           lkf_rtcp_ref *refs, uint32_t ref_cap, uint32_t *n_refs, uint32_t *n_nacks) {
  if (!e || !n_fb || !n_refs || (n && (!in || !out)) || (fb_cap && (!fb || !fb_out)) || (ref_cap && !refs) ||
      (arena_len && !arena && !dArena))
    return LKF_EINVAL;
  *n_fb = *n_refs = 0;
  if (n_nacks) *n_nacks = 0;
  // groups: one per DownTrack's contiguous entries (a DownTrack must not reappear)
  std::vector<uint32_t> g;
  if (n)
    STEP(check_handles(&in[0].dt, sizeof(*in), n, e->dtp.size(), {Repeat::Groups, &g, true}, [&](uint32_t i) {
      return in[i].len <= LKF_RTCP_MAX_LEN && uint64_t(in[i].off) + in[i].len <= arena_len;
    }));
  const uint32_t ngroups = n ? uint32_t(g.size() - 1) : 0;
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  hipStream_t s = f.s;
  e->riNacks = 0;  // the last call's NACK list ends here
  e->riGroups.clear();
  if (!n) return LKF_OK;
  // The per-entry buffers are one family, sized for twice the entries; the
  // scan state is zeroed once, on the call's stream, when it is reallocated.
  const uint64_t m = 2 * uint64_t(n);
  auto words = [](uint64_t k) {
    return uint64_t(scan_state_words(uint32_t(std::min<uint64_t>(std::max<uint64_t>(k, 4096), 0xffffffffu))));
  };
  STEP(f.grow("alloc rtcp ingress scratch", want(e->dRiIn, n, 4096, m), want(e->dRiGEntry, uint64_t(n) + 1, 4097, m + 1),
              want(e->dRiFbG, uint64_t(n) + 1, 4097, m + 1), want(e->dRiFbCnt, n, 4096, m),
              want(e->dRiRefCnt, n, 4096, m), want(e->dRiNackCnt, n, 4096, m), want(e->dRiFbOff, n, 4096, m),
              want(e->dRiNackOff, n, 4096, m), want(e->dRiRes, n, 4096, m), want(e->dRiTot, 4, 4),
              want(e->dRiScan, words(n), 0, words(m)), want(e->dRiRefOff, n, 4096, m)));
  if (f.grew) HIPCHK(hipMemsetAsync(e->dRiScan, 0, e->dRiScan.cap() * sizeof(uint64_t), s), "rtcp scan state reset");
  if (arena) STEP(f.grow("alloc rtcp arena", want(e->dRiArena, arena_len, 1 << 16, 2 * arena_len)));  // (a family of its own)
  STEP(f.up(e->dRiIn, in, size_t(n) * sizeof(lkf_rtcp_raw), "rtcp raw copy"));
  if (arena && arena_len) STEP(f.up(e->dRiArena, arena, arena_len, "rtcp arena copy"));
  STEP(f.up(e->dRiGEntry, g.data(), g.size() * sizeof(uint32_t), "rtcp groups copy"));
  RtcpInLaunch a{};
  a.in = e->dRiIn;
  a.n = n;
  a.arena = arena ? e->dRiArena.get() : dArena;
  a.arenaLen = arena_len;
  a.dts = e->dDTs;
  a.hot = e->dHot;
  a.ndts = uint32_t(e->dtp.size());
  a.res = e->dRiRes;
  a.fbCnt = e->dRiFbCnt;
  a.refCnt = e->dRiRefCnt;
  a.nackCnt = e->dRiNackCnt;
  a.fbOff = e->dRiFbOff;
  a.nackOff = e->dRiNackOff;
  a.refOff = e->dRiRefOff;
  a.totals = e->dRiTot;
  a.gEntry = e->dRiGEntry;
  a.ngroups = ngroups;
  a.fbG = e->dRiFbG;
  HIPCHK(launch_rtcp_in_count(s, a), "rtcp count");
  // input-order offsets: (fb records, sequence numbers) in one scan, the refs in another
  HIPCHK(launch_scan(s, 1, nullptr, nullptr, nullptr, e->dRiFbCnt, e->dRiNackCnt, n, e->dRiScan, nullptr, e->dRiFbOff,
                     e->dRiNackOff, e->dRiTot, e->dRiTot + 1, nullptr),
         "rtcp scan");
  HIPCHK(launch_scan(s, 2, nullptr, nullptr, nullptr, e->dRiRefCnt, nullptr, n, e->dRiScan, nullptr, e->dRiRefOff,
                     nullptr, e->dRiTot + 2, nullptr, nullptr),
         "rtcp ref scan");
  uint64_t tot[3] = {};
  STEP(f.down(tot, e->dRiTot, sizeof(tot), "rtcp totals copy"));
  STEP(f.wait());
  for (uint64_t t : tot)
    if (t > 0xffffffffull) {  // (or a scan that gave up: ~0)
      e->err = "RTCP ingest: a list of one call exceeds 2^32 - 1 records";
      return LKF_EINVAL;
    }
  // the lists, sized by the counts (the stream is idle here)
  HIPCHK(e->dRiFb.reserve(tot[0], 4096), "alloc rtcp fb");
  HIPCHK(e->dRiFbOut.reserve(tot[0], 4096), "alloc rtcp fb results");
  HIPCHK(e->dRiNacks.reserve(tot[1], 4096), "alloc rtcp nacks");
  HIPCHK(e->dRiRefs.reserve(tot[2], 1024), "alloc rtcp refs");
  a.fb = e->dRiFb;
  a.nacks = e->dRiNacks;
  a.refs = e->dRiRefs;
  a.fbCap = tot[0];
  a.nackCap = tot[1];
  a.refCap = tot[2];
  a.fbOut = e->dRiFbOut;
  HIPCHK(launch_rtcp_in_write(s, a), "rtcp write");
  RrUpdateLaunch u;
  u.in = e->dRiFb;
  u.gBegin = e->dRiFbG;
  u.ngroups = ngroups;
  u.n = uint32_t(tot[0]);
  u.now = now_ns;
  u.ss = e->dSS;
  u.ring = e->dSSRing;
  u.rtcp = e->dRtcp;
  u.ndts = uint32_t(e->dtp.size());
  u.out = e->dRiFbOut;
  HIPCHK(launch_rr_update(s, u), "rr update");
  HIPCHK(launch_rtcp_in_fold(s, a), "rtcp fold");
  STEP(f.wait());
  D2H(out, e->dRiRes, size_t(n) * sizeof(lkf_rtcp_in_result), "rtcp results copy");
  *n_fb = uint32_t(tot[0]);
  *n_refs = uint32_t(tot[2]);
  if (n_nacks) *n_nacks = uint32_t(tot[1]);
  // each DownTrack's share of the NACK list, for lkf_rtx_lookup_ingested
  e->riNacks = uint32_t(tot[1]);
  for (uint32_t k = 0; k < ngroups; k++) {
    const uint32_t b = out[g[k]].nack_first, en = k + 1 < ngroups ? out[g[k + 1]].nack_first : uint32_t(tot[1]);
    if (en > b) e->riGroups.push_back({in[g[k]].dt, b, en});
  }
  if (tot[0] > fb_cap || tot[2] > ref_cap) return LKF_ENOSPC;
  if (tot[0]) {
    D2H(fb, e->dRiFb, size_t(tot[0]) * sizeof(lkf_rtcp_fb), "rtcp fb copy");
    D2H(fb_out, e->dRiFbOut, size_t(tot[0]) * sizeof(lkf_rtcp_fb_result), "rtcp fb results copy");
  }
  if (tot[2]) D2H(refs, e->dRiRefs, size_t(tot[2]) * sizeof(lkf_rtcp_ref), "rtcp refs copy");
  return LKF_OK;
}

int lkf_rtcp_ingest(lkf_engine *e, const lkf_rtcp_raw *in, uint32_t n, const uint8_t *arena, uint64_t arena_len,
                    int64_t now_ns, lkf_rtcp_in_result *out, lkf_rtcp_fb *fb, lkf_rtcp_fb_result *fb_out,
                    uint32_t fb_cap, uint32_t *n_fb, lkf_rtcp_ref *refs, uint32_t ref_cap, uint32_t *n_refs,
                    uint32_t *n_nacks) {
  if (arena_len && !arena) return LKF_EINVAL;
  static const uint8_t none = 0;  // (an empty arena is still the caller's)
  return rtcp_ingest_run(e, in, n, arena ? arena : &none, nullptr, arena_len, now_ns, out, fb, fb_out, fb_cap, n_fb, refs,
                         ref_cap, n_refs, n_nacks);
}

int lkf_rtcp_ingested_nacks(lkf_engine *e, lkf_nack *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = e->riNacks;
  if (cap < e->riNacks) return LKF_ENOSPC;
  if (!e->riNacks) return LKF_OK;
  if (!out) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  D2H(out, e->dRiNacks, size_t(e->riNacks) * sizeof(lkf_nack), "rtcp nacks copy");  // (the ingest left its stream idle)
  return LKF_OK;
}

int lkf_rtx_lookup_ingested(lkf_engine *e, int64_t now_ns, lkf_rtx *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = 0;
  e->rtxNow = now_ns;
  // k_rtx_lookup's groups are non-empty and contiguous: the DownTracks without
  // a NACK are not in riGroups, and while no listed DownTrack has been removed
  // the list is looked up where the ingest wrote it.  Otherwise the kept
  // DownTracks' shares are packed device to device into the lookup's own list.
  std::vector<uint32_t> gb;
  std::vector<const lkf_engine::RiGroup *> keep;
  uint32_t m = 0;
  for (const auto &q : e->riGroups)
    if (e->active[q.dt]) {  // a removed DownTrack answers no NACK
      keep.push_back(&q);
      gb.push_back(m);
      m += q.end - q.begin;
    }
  if (keep.empty()) return LKF_OK;
  gb.push_back(m);
  const bool inPlace = keep.size() == e->riGroups.size();
  Frame f(e, Order::BehindDecide);  // as lkf_rtx_lookup: behind the queued decides
  STEP(f.open());
  HIPCHK(hipEventRecord(e->inEv, e->sendS), "event");  // the ingest's write pass
  HIPCHK(hipStreamWaitEvent(f.s, e->inEv, 0), "wait sender stream");
  STEP(rtx_grow(f, m));
  if (!inPlace)
    for (size_t k = 0; k < keep.size(); k++)
      HIPCHK(hipMemcpyAsync(e->dNacks + gb[k], e->dRiNacks + keep[k]->begin,
                            size_t(keep[k]->end - keep[k]->begin) * sizeof(lkf_nack), hipMemcpyDeviceToDevice, f.s),
             "nacks pack");
  STEP(f.up(e->dNackG, gb.data(), gb.size() * sizeof(uint32_t), "groups copy"));
  return rtx_lookup_run(f, inPlace ? e->dRiNacks.get() : e->dNacks.get(), uint32_t(keep.size()), m, now_ns, out, cap,
                        n_out);
}

// ---- SRTCP (srtp_kernels.hip k_srtcp_*; the receive steps are srtcp_device.h) ----
static_assert(sizeof(lkf_srtcp_raw) == 12 && sizeof(lkf_srtcp_rx_result) == 16 && sizeof(lkf_rtcp_entry) == 8 &&
                  sizeof(lkf_transport_srtcp) == 368 && sizeof(lkf_srtcp_tx_result) == 16,
              "SRTCP records");

// Control-rate, the RTCP calls' frame (Order::BehindSender).  The datagrams go
// into the engine's own staging, padded so that the kernels' 16-B reads of a
// datagram's last chunk stay inside it; the plaintext arena stays on the device.
int lkf_srtcp_unprotect(lkf_engine *e, const lkf_srtcp_raw *in, uint32_t n, const uint8_t *srtcp, uint64_t srtcp_len,
                        uint8_t *plain, lkf_srtcp_rx_result *out) {
  if (!e || (n && (!in || !out)) || (srtcp_len && !srtcp)) return LKF_EINVAL;
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  e->scOff.assign(n, 0);
  e->scLen.assign(n, 0);
  e->scTransport.assign(n, -1);
  e->scOnDevice = false;
  e->scPlainLen = srtcp_len;
  if (!n) return LKF_OK;
  for (uint32_t i = 0; i < n; i++) e->scOff[i] = in[i].off, e->scTransport[i] = in[i].transport;
  if (e->transports.empty()) {  // every handle is unknown
    for (uint32_t i = 0; i < n; i++) out[i] = lkf_srtcp_rx_result{0, 0, LKF_SRTCP_RX_MALFORMED, 0};
    return LKF_OK;
  }
  STEP(f.grow("alloc srtcp rx scratch", want(e->dScIn, n, 4096, 2 * uint64_t(n)),
              want(e->dScSpec, n, 4096, 2 * uint64_t(n)), want(e->dScAuth, n, 4096, 2 * uint64_t(n)),
              want(e->dScRes, n, 4096, 2 * uint64_t(n))));
  STEP(f.grow("alloc srtcp arenas", want(e->dScArena, srtcp_len + 64, 1 << 16, 2 * srtcp_len + 64),
              want(e->dScPlain, srtcp_len + 64, 1 << 16, 2 * srtcp_len + 64)));
  STEP(f.up(e->dScIn, in, size_t(n) * sizeof(lkf_srtcp_raw), "srtcp raw copy"));
  if (srtcp_len) STEP(f.up(e->dScArena, srtcp, srtcp_len, "srtcp arena copy"));
  SrtcpRxArgs a{};
  a.tab = e->dAesTab;
  a.in = e->dScIn;
  a.n = n;
  a.ntransports = uint32_t(e->transports.size());
  a.srtcp = e->dScArena;
  a.srtcpLen = srtcp_len;
  a.plain = e->dScPlain;
  a.rx = e->dSrtcpRx;
  a.rxSpec = e->dSrtcpRxSpec;
  a.range = e->dSrtcpRange;
  a.keys = e->dSrtcpKeys;
  a.spec = e->dScSpec;
  a.auth = e->dScAuth;
  a.res = e->dScRes;
  HIPCHK(launch_srtcp_unprotect(f.s, a), "srtcp unprotect");
  STEP(f.wait());
  D2H(out, e->dScRes, size_t(n) * sizeof(lkf_srtcp_rx_result), "srtcp results copy");
  if (plain && srtcp_len) D2H(plain, e->dScPlain, srtcp_len, "srtcp plaintext copy");
  for (uint32_t i = 0; i < n; i++) e->scLen[i] = out[i].len;
  e->scOnDevice = true;
  return LKF_OK;
}

int lkf_rtcp_ingest_unprotected(lkf_engine *e, const lkf_rtcp_entry *in, uint32_t n, int64_t now_ns,
                                lkf_rtcp_in_result *out, lkf_rtcp_fb *fb, lkf_rtcp_fb_result *fb_out, uint32_t fb_cap,
                                uint32_t *n_fb, lkf_rtcp_ref *refs, uint32_t ref_cap, uint32_t *n_refs,
                                uint32_t *n_nacks) {
  if (!e || (n && !in)) return LKF_EINVAL;
  std::vector<lkf_rtcp_raw> raw(n);
  for (uint32_t i = 0; i < n; i++) {
    if (in[i].dgram >= e->scOff.size()) return LKF_EINVAL;
    const uint32_t len = e->scLen[in[i].dgram];  // (a rejected datagram: an empty entry at the arena's start)
    raw[i] = lkf_rtcp_raw{in[i].dt, len ? e->scOff[in[i].dgram] : 0u, len};
  }
  static const uint8_t none = 0;  // (no datagram was accepted yet: every entry has len 0)
  const uint8_t *host = e->dScPlain ? nullptr : &none;
  return rtcp_ingest_run(e, raw.data(), n, host, e->dScPlain, host ? 0 : e->scPlainLen, now_ns, out, fb, fb_out, fb_cap,
                         n_fb, refs, ref_cap, n_refs, n_nacks);
}

// ---- RTCP demultiplexing (rtcp_kernels.hip k_rtcp_dmx_*; the walk is rtcp_dmx_device.h) ----
static_assert(sizeof(lkf_rtcp_dmx_result) == 16, "RTCP demux records");

// The routing table from the host's lists: the active DownTracks with a
// receive transport, one row per (transport, SSRC), the highest handle of a
// key kept; its CSR by transport; the rows in ascending DownTrack order.
// Uploaded on the call's stream (the family grows only here, so the table
// stays on the device until it is dirty again).
static int rtcp_dmx_rebuild(lkf_engine *e, Frame &f) {
  std::vector<RtcpDmxRow> rows;
  for (size_t d = 0; d < e->dtp.size(); d++)
    if (e->active[d] && e->dtRtcpTransport[d] >= 0)
      rows.push_back({uint32_t(e->dtRtcpTransport[d]), e->dtp[d].ssrc, int32_t(d)});
  std::sort(rows.begin(), rows.end(), [](const RtcpDmxRow &a, const RtcpDmxRow &b) {
    return std::tie(a.transport, a.ssrc, a.dt) < std::tie(b.transport, b.ssrc, b.dt);
  });
  size_t k = 0;
  for (size_t i = 0; i < rows.size(); i++)  // the last of a key's run: the highest handle
    if (i + 1 == rows.size() || rows[i + 1].transport != rows[i].transport || rows[i + 1].ssrc != rows[i].ssrc)
      rows[k++] = rows[i];
  rows.resize(k);
  const size_t nt = e->transports.size();
  std::vector<uint32_t> tFirst(nt + 1, 0), byDt(rows.size());
  for (const auto &r : rows) tFirst[r.transport + 1]++;
  for (size_t t = 0; t < nt; t++) tFirst[t + 1] += tFirst[t];
  for (size_t i = 0; i < byDt.size(); i++) byDt[i] = uint32_t(i);
  std::sort(byDt.begin(), byDt.end(), [&](uint32_t a, uint32_t b) { return rows[a].dt < rows[b].dt; });
  const uint64_t nr = rows.size(), m = 2 * nr;
  auto words = [](uint64_t q) {
    return uint64_t(scan_state_words(uint32_t(std::min<uint64_t>(std::max<uint64_t>(q, 4096), 0xffffffffu))));
  };
  STEP(f.grow("alloc rtcp demux table", want(e->dDmxRows, nr, 1024, m), want(e->dDmxByDt, nr, 1024, m),
              want(e->dDmxCnt, nr, 1024, m), want(e->dDmxOff, nr, 1024, m), want(e->dDmxTFirst, nt + 1, 256, 2 * nt + 1),
              want(e->dDmxTdFirst, nt + 1, 256, 2 * nt + 1), want(e->dDmxTot, 1, 1),
              want(e->dDmxScan, words(nr), 0, words(m))));
  if (f.grew)
    HIPCHK(hipMemsetAsync(e->dDmxScan, 0, e->dDmxScan.cap() * sizeof(uint64_t), f.s), "rtcp demux scan state reset");
  if (nr) {
    STEP(f.up(e->dDmxRows, rows.data(), nr * sizeof(RtcpDmxRow), "rtcp demux rows copy"));
    STEP(f.up(e->dDmxByDt, byDt.data(), nr * sizeof(uint32_t), "rtcp demux order copy"));
  }
  STEP(f.up(e->dDmxTFirst, tFirst.data(), tFirst.size() * sizeof(uint32_t), "rtcp demux csr copy"));
  STEP(f.wait());  // (the uploads read this function's vectors)
  e->dmxTFirst = std::move(tFirst);
  e->dmxRows = uint32_t(nr);
  e->dmxDirty = false;
  return LKF_OK;
}

// The two calls' body.  tr / len: each datagram's transport and plaintext
// length on the host (an empty datagram's transport is not looked at).  `in`:
// the list in host memory, uploaded with `arena`; NULL: the list is dIn with
// the lengths in dRx, the bytes the arena_len at dArena (the last unprotect's).
// Mark pass -> count pass -> scan -> the total back on the host (the entry
// list is sized by it) -> write pass.
static int rtcp_dmx_run(lkf_engine *e, const int32_t *tr, const uint32_t *len, uint32_t n, const lkf_srtcp_raw *in,
                        const uint8_t *arena, const lkf_srtcp_raw *dIn, const lkf_srtcp_rx_result *dRx,
                        const uint8_t *dArena, uint64_t arena_len, lkf_rtcp_dmx_result *res, lkf_rtcp_entry *entries,
                        uint32_t cap, uint32_t *n_entries) {
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  if (!n) return LKF_OK;
  const size_t nt = e->transports.size();
  if (e->dmxDirty || e->dmxTFirst.size() != nt + 1) STEP(rtcp_dmx_rebuild(e, f));
  // each datagram's bitmap row and each transport's datagrams, in call order
  std::vector<uint32_t> bmOff(size_t(n) + 1, 0), tdFirst(nt + 1, 0), tdList;
  uint64_t bmWords = 0;
  auto live = [&](uint32_t i) { return len[i] && tr[i] >= 0 && size_t(tr[i]) < nt; };
  for (uint32_t i = 0; i < n; i++) {
    if (live(i)) {
      bmWords += (e->dmxTFirst[size_t(tr[i]) + 1] - e->dmxTFirst[size_t(tr[i])] + 31) / 32;
      tdFirst[size_t(tr[i]) + 1]++;
    }
    if (bmWords > 0xffffffffull) {
      e->err = "RTCP demux: the bitmap rows of one call exceed 2^32 - 1 words";
      return LKF_EINVAL;
    }
    bmOff[size_t(i) + 1] = uint32_t(bmWords);
  }
  for (size_t t = 0; t < nt; t++) tdFirst[t + 1] += tdFirst[t];
  tdList.resize(tdFirst[nt]);
  {
    std::vector<uint32_t> at(tdFirst.begin(), tdFirst.end() - 1);
    for (uint32_t i = 0; i < n; i++)
      if (live(i)) tdList[at[size_t(tr[i])]++] = i;
  }
  const uint64_t m = 2 * uint64_t(n);
  STEP(f.grow("alloc rtcp demux scratch", want(e->dDmxIn, n, 4096, m), want(e->dDmxBmOff, uint64_t(n) + 1, 4097, m + 1),
              want(e->dDmxTdList, n, 4096, m), want(e->dDmxRes, n, 4096, m)));
  STEP(f.grow("alloc rtcp demux bitmap", want(e->dDmxBits, bmWords, 4096, 2 * bmWords)));
  if (in) {
    STEP(f.grow("alloc rtcp demux arena", want(e->dDmxArena, arena_len, 1 << 16, 2 * arena_len)));
    STEP(f.up(e->dDmxIn, in, size_t(n) * sizeof(lkf_srtcp_raw), "rtcp demux list copy"));
    if (arena_len) STEP(f.up(e->dDmxArena, arena, arena_len, "rtcp demux arena copy"));
  }
  STEP(f.up(e->dDmxBmOff, bmOff.data(), bmOff.size() * sizeof(uint32_t), "rtcp demux bitmap rows copy"));
  STEP(f.up(e->dDmxTdFirst, tdFirst.data(), tdFirst.size() * sizeof(uint32_t), "rtcp demux ranges copy"));
  if (!tdList.empty())
    STEP(f.up(e->dDmxTdList, tdList.data(), tdList.size() * sizeof(uint32_t), "rtcp demux datagram lists copy"));
  if (bmWords) HIPCHK(hipMemsetAsync(e->dDmxBits, 0, bmWords * sizeof(uint32_t), f.s), "rtcp demux bitmap reset");
  RtcpDmxLaunch a{};
  a.in = in ? e->dDmxIn.get() : dIn;
  a.rx = in ? nullptr : dRx;
  a.n = n;
  a.arena = in ? e->dDmxArena.get() : dArena;
  a.arenaLen = arena_len;
  a.rows = e->dDmxRows;
  a.nrows = e->dmxRows;
  a.tFirst = e->dDmxTFirst;
  a.ntransports = uint32_t(nt);
  a.byDt = e->dDmxByDt;
  a.bmOff = e->dDmxBmOff;
  a.bits = e->dDmxBits;
  a.bmWords = bmWords;
  a.tdFirst = e->dDmxTdFirst;
  a.tdList = e->dDmxTdList;
  a.res = e->dDmxRes;
  a.cnt = e->dDmxCnt;
  a.off = e->dDmxOff;
  HIPCHK(launch_rtcp_dmx_mark(f.s, a), "rtcp demux mark");
  uint64_t total = 0;
  if (a.nrows) {
    HIPCHK(launch_rtcp_dmx_count(f.s, a), "rtcp demux count");
    HIPCHK(launch_scan(f.s, 2, nullptr, nullptr, nullptr, e->dDmxCnt, nullptr, a.nrows, e->dDmxScan, nullptr, e->dDmxOff,
                       nullptr, e->dDmxTot, nullptr, nullptr),
           "rtcp demux scan");
    STEP(f.down(&total, e->dDmxTot, sizeof(total), "rtcp demux total copy"));
  }
  STEP(f.wait());
  D2H(res, e->dDmxRes, size_t(n) * sizeof(lkf_rtcp_dmx_result), "rtcp demux results copy");
  if (total > 0xffffffffull) {  // (or a scan that gave up: ~0)
    e->err = "RTCP demux: one call yields more than 2^32 - 1 entries";
    return LKF_EINVAL;
  }
  *n_entries = uint32_t(total);
  if (total > cap) return LKF_ENOSPC;
  if (!total) return LKF_OK;
  HIPCHK(e->dDmxEntries.reserve(total, 4096), "alloc rtcp demux entries");  // (the stream is idle here)
  a.entries = e->dDmxEntries;
  a.entryCap = total;
  HIPCHK(launch_rtcp_dmx_write(f.s, a), "rtcp demux write");
  STEP(f.wait());
  D2H(entries, e->dDmxEntries, size_t(total) * sizeof(lkf_rtcp_entry), "rtcp demux entries copy");
  return LKF_OK;
}

int lkf_rtcp_demux_unprotected(lkf_engine *e, lkf_rtcp_dmx_result *res, lkf_rtcp_entry *entries, uint32_t cap,
                               uint32_t *n_entries) {
  if (!e || !n_entries) return LKF_EINVAL;
  *n_entries = 0;
  const uint32_t n = uint32_t(e->scLen.size());
  if ((n && !res) || (cap && !entries)) return LKF_EINVAL;
  for (uint32_t i = 0; i < n; i++)
    if (e->scLen[i] > LKF_RTCP_MAX_LEN) return LKF_EINVAL;  // (as lkf_rtcp_ingest_unprotected would)
  if (!e->scOnDevice) {  // no datagram of that call reached the device: every one was rejected
    for (uint32_t i = 0; i < n; i++) res[i] = lkf_rtcp_dmx_result{LKF_RTCP_DMX_EMPTY, 0, 0, 0};
    return LKF_OK;
  }
  return rtcp_dmx_run(e, e->scTransport.data(), e->scLen.data(), n, nullptr, nullptr, e->dScIn, e->dScRes, e->dScPlain,
                      e->scPlainLen, res, entries, cap, n_entries);
}

int lkf_rtcp_demux(lkf_engine *e, const lkf_srtcp_raw *in, uint32_t n, const uint8_t *arena, uint64_t arena_len,
                   lkf_rtcp_dmx_result *res, lkf_rtcp_entry *entries, uint32_t cap, uint32_t *n_entries) {
  if (!e || !n_entries || (n && (!in || !res)) || (cap && !entries) || (arena_len && !arena)) return LKF_EINVAL;
  *n_entries = 0;
  std::vector<int32_t> tr(n);
  std::vector<uint32_t> len(n);
  for (uint32_t i = 0; i < n; i++) {
    if (in[i].transport < 0 || in[i].transport >= int32_t(e->transports.size()) || in[i].len > LKF_RTCP_MAX_LEN ||
        uint64_t(in[i].off) + in[i].len > arena_len)
      return LKF_EINVAL;
    tr[i] = in[i].transport;
    len[i] = in[i].len;
  }
  static const uint8_t none = 0;  // (an empty arena is still the caller's)
  return rtcp_dmx_run(e, tr.data(), len.data(), n, in, arena ? arena : &none, nullptr, nullptr, nullptr, arena_len, res,
                      entries, cap, n_entries);
}

int lkf_transport_srtcp_get(lkf_engine *e, int32_t transport, lkf_transport_srtcp *out) {
  if (!e || !out || transport < 0 || transport >= int32_t(e->transports.size())) return LKF_EINVAL;
  STEP(quiesce(e, false));
  D2H(out, e->dSrtcpRx + transport, sizeof(*out), "srtcp rx state copy");
  return LKF_OK;
}

int lkf_srtcp_reset(lkf_engine *e, int32_t transport) {
  if (!e || transport < 0 || transport >= int32_t(e->transports.size())) return LKF_EINVAL;
  STEP(quiesce(e, false));
  HIPCHK(hipMemset(e->dSrtcpRx + transport, 0, sizeof(lkf_transport_srtcp)), "srtcp rx reset");
  e->scTxIndex.erase(e->scTxIndex.lower_bound({transport, 0u}), e->scTxIndex.upper_bound({transport, 0xffffffffu}));
  return upload_done(e);
}

// The index counters live here: the input is trusted and host-resident, and a
// call that fails its checks must consume none.
int lkf_srtcp_protect(lkf_engine *e, const lkf_srtcp_raw *in, uint32_t n, const uint8_t *plain, uint64_t plain_len,
                      uint8_t *out, uint64_t out_cap, lkf_srtcp_tx_result *res, uint64_t *out_len) {
  if (!e || (n && (!in || !plain || !res))) return LKF_EINVAL;
  uint64_t total = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (in[i].transport < 0 || in[i].transport >= int32_t(e->transports.size()) || in[i].len < 8 ||
        uint64_t(in[i].off) + in[i].len > plain_len || (plain[in[i].off] >> 6) != 2)
      return LKF_EINVAL;
    total += (uint64_t(in[i].len) + 20 + 15) & ~15ull;
  }
  if (out_len) *out_len = total;
  if (total > 0xffffffffull) return LKF_EINVAL;
  if (total > out_cap || (total && !out)) return LKF_ENOSPC;
  if (!n) return LKF_OK;
  // the plaintext laid out where the protected packets go, zeros between
  std::vector<uint8_t> stage(total, 0);
  std::vector<SrtcpTx> tx(n);
  uint64_t off = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t *p = plain + in[i].off;
    std::memcpy(stage.data() + off, p, in[i].len);
    const uint32_t ssrc = (uint32_t(p[4]) << 24) | (uint32_t(p[5]) << 16) | (uint32_t(p[6]) << 8) | p[7];
    uint32_t &idx = e->scTxIndex[{in[i].transport, ssrc}];
    idx = (idx + 1) & 0x7fffffffu;  // pion's srtcpIndex++ before use
    const bool gcm = e->transports[size_t(in[i].transport)].profile == LKF_SRTP_AEAD_AES_128_GCM;
    tx[i] = SrtcpTx{uint32_t(in[i].transport), uint32_t(off), in[i].len, idx};
    res[i] = lkf_srtcp_tx_result{ssrc, idx, uint32_t(off), in[i].len + (gcm ? 20u : 14u)};
    off += (uint64_t(in[i].len) + 20 + 15) & ~15ull;
  }
  Frame f(e, Order::BehindSender);
  STEP(f.open());
  STEP(f.grow("alloc srtcp tx scratch", want(e->dScTx, n, 1024, 2 * uint64_t(n)),
              want(e->dScTxIn, total, 1 << 16, 2 * total), want(e->dScTxOut, total, 1 << 16, 2 * total)));
  STEP(f.up(e->dScTx, tx.data(), size_t(n) * sizeof(SrtcpTx), "srtcp tx copy"));
  STEP(f.up(e->dScTxIn, stage.data(), total, "srtcp plaintext copy"));
  HIPCHK(hipMemsetAsync(e->dScTxOut, 0, total, f.s), "srtcp out clear");  // (the slack behind each packet reads 0)
  SrtcpTxArgs a{};
  a.tab = e->dAesTab;
  a.pk = e->dScTx;
  a.n = n;
  a.src = e->dScTxIn;
  a.dst = e->dScTxOut;
  a.keys = e->dSrtcpKeys;
  HIPCHK(launch_srtcp_protect(f.s, a), "srtcp protect");
  STEP(f.wait());  // (also: the pageable uploads above have left the host vectors)
  D2H(out, e->dScTxOut, total, "srtcp protected copy");
  return LKF_OK;
}

int lkf_srtcp_tx_index(lkf_engine *e, int32_t transport, uint32_t ssrc, uint32_t *index) {
  if (!e || !index || transport < 0 || transport >= int32_t(e->transports.size())) return LKF_EINVAL;
  const auto it = e->scTxIndex.find({transport, ssrc});
  *index = it == e->scTxIndex.end() ? 0 : it->second;
  return LKF_OK;
}

static int rtx_emit_common(Frame &f, const lkf_rtx *rtx, uint32_t n, const uint8_t *srcArena,
                           const std::vector<uint16_t> &srcHdr, lkf_out *out, uint8_t *out_arena, uint64_t out_cap,
                           uint32_t *n_out, uint64_t *out_len);
// The retransmissions run on the sender stream (Order::BehindSender), after
// every queued stage that touches what they read or update: the decides and
// sequencer DD bytes (decide stream), the sender statistics (sender stream for
// long batches, emit stream for short ones — the RTX sendingPacket updates
// the same RTPStatsSender) and the bucket copies (sender stream).  The host
// then waits for that point: the scratch buffers are rewritten from the host.
static int rtx_open(Frame &f, uint32_t n) {
  STEP(f.open(true, true));
  STEP(f.wait());
  return rtx_grow(f, n);
}
int lkf_rtx_emit(lkf_engine *e, const lkf_rtx *rtx, uint32_t n, const lkf_raw_pkt *src, const uint8_t *src_arena,
                 uint64_t src_len, lkf_out *out, uint8_t *out_arena, uint64_t out_cap, uint32_t *n_out,
                 uint64_t *out_len) {
  if (!e || !n_out || !out_len || (n && (!rtx || !src))) return LKF_EINVAL;
  *n_out = 0;
  *out_len = 0;
  if (!n) return LKF_OK;
  STEP(check_handles(&rtx[0].dt, sizeof(*rtx), n, e->dtp.size(), {}, [&](uint32_t i) {
    return !src[i].len || (src_arena && uint64_t(src[i].off) + src[i].len <= src_len);
  }));
  Frame f(e, Order::BehindSender);
  STEP(rtx_open(f, n));
  HIPCHK(e->dRtxIn.reserve(src_len + 64, 1 << 20), "alloc rtx in");  // (the stream is idle)
  // uploads ordered on the sender stream ahead of the kernels that read them
  // (a pageable hipMemcpy may return before its DMA lands, and the engine's
  // streams do not order against the null stream)
  STEP(f.up(e->dRtx, rtx, n * sizeof(lkf_rtx), "rtx copy"));
  STEP(f.up(e->dRtxSrc, src, n * sizeof(lkf_raw_pkt), "src copy"));
  if (src_len) STEP(f.up(e->dRtxIn, src_arena, src_len, "src arena copy"));
  std::vector<uint16_t> hdr(n, 0);
  for (uint32_t i = 0; i < n; i++) {
    if (!src[i].len) continue;
    const uint8_t *b = src_arena + src[i].off;
    uint32_t h = 12 + 4 * (b[0] & 0xf);
    if ((b[0] & 0x10) && h + 4 <= src[i].len) h += 4 + 4 * ((uint32_t(b[h + 2]) << 8) | b[h + 3]);
    hdr[i] = uint16_t(h);
  }
  return rtx_emit_common(f, rtx, n, e->dRtxIn, hdr, out, out_arena, out_cap, n_out, out_len);
}

// The retransmissions from device-side sources (dRtx / dRtxSrc filled; srcArena:
// the bytes they index): sizes, offsets, wire bytes, then sendingPacket per
// retransmission (srcHdr[i]: the source header's size).
static int rtx_emit_common(Frame &f, const lkf_rtx *rtx, uint32_t n, const uint8_t *srcArena,
                           const std::vector<uint16_t> &srcHdr, lkf_out *out, uint8_t *out_arena, uint64_t out_cap,
                           uint32_t *n_out, uint64_t *out_len) {
  lkf_engine *e = f.e;
  const uint8_t *rtxDD = nullptr;
  if (e->nSeqDD) {  // epm.ddBytes of each record (its sequencer slot)
    HIPCHK(e->dRtxDD.reserve(size_t(n) * kSeqDDBytes, 1024 * kSeqDDBytes), "alloc rtx dd");
    HIPCHK(launch_rtx_dd(e->sendS, n, e->dRtx, e->dDTs, e->dSeq, e->cfg.seq_size, e->dSeqDDIdx, e->dSeqDD,
                         e->dRtxDD),
           "rtx dd");
    rtxDD = e->dRtxDD;
  }
  HIPCHK(launch_rtx_emit(e->sendS, false, n, e->dRtx, e->dRtxSrc, srcArena, e->dDTs, e->dTracks, e->dRtxLen,
                         nullptr, nullptr, rtxDD),
         "rtx size");
  std::vector<uint32_t> len(n);
  STEP(f.down(len.data(), e->dRtxLen, n * sizeof(uint32_t), "len copy"));
  STEP(f.wait());
  std::vector<uint64_t> off(n, 0);
  uint64_t tot = 0;
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; i++) {
    off[i] = tot;
    if (len[i]) {
      tot += (uint64_t(len[i]) + 15) & ~uint64_t(15);
      k++;
    }
  }
  *n_out = k;
  *out_len = tot;
  if (tot > out_cap || (k && (!out || !out_arena))) return LKF_ENOSPC;
  HIPCHK(e->dRtxOut.reserve(tot + 64, 1 << 20), "alloc rtx out");  // (the stream is idle)
  STEP(f.up(e->dRtxOff, off.data(), n * sizeof(uint64_t), "off copy"));
  HIPCHK(launch_rtx_emit(e->sendS, true, n, e->dRtx, e->dRtxSrc, srcArena, e->dDTs, e->dTracks, e->dRtxLen,
                         e->dRtxOff, e->dRtxOut, rtxDD),
         "rtx write");
  if (e->anyTwcc)  // transport-cc numbers in record (send) order
    HIPCHK(launch_twcc_stamp(e->sendS, e->dDTs, e->dTwccCtrD, e->dTwccCtrT, n, nullptr, nullptr, nullptr, e->dRtx,
                             e->dRtxOff, e->dRtxLen, e->dRtxOut),
           "twcc stamp");
  if (tot) STEP(f.down(out_arena, e->dRtxOut, tot, "rtx bytes copy"));
  STEP(f.wait());
  {  // sendingPacket (downtrack.go:1671-1681): the bucket packet's header as
     // unmarshalled (CSRCs and extensions kept), the forwarded payload
    std::vector<SenderUpd> ul;
    for (uint32_t i = 0; i < n; i++) {
      if (!len[i]) continue;
      const uint32_t h = srcHdr[i];
      const uint8_t *w = out_arena + off[i];  // the RTX header as written (CSRCs, pacer extension block)
      uint32_t outHdr = 12 + 4 * uint32_t(w[0] & 0xf);
      if (w[0] & 0x10) outHdr += 4 + 4 * ((uint32_t(w[outHdr + 2]) << 8) | w[outHdr + 3]);
      SenderUpd u;
      std::memset(&u, 0, sizeof(u));
      u.esn = rtx[i].meta.ext_sn;
      u.ets = rtx[i].meta.ext_ts;
      u.t = e->rtxNow;
      u.dt = uint32_t(rtx[i].dt);
      u.hdr = uint16_t(h);
      u.pay = uint16_t(len[i] - outHdr);
      u.marker = rtx[i].meta.marker ? 1 : 0;
      ul.push_back(u);
    }
    STEP(sender_list(e, ul));
  }
  k = 0;
  for (uint32_t i = 0; i < n; i++) {
    if (!len[i]) continue;
    lkf_out &o = out[k++];
    std::memset(&o, 0, sizeof(o));
    o.ext_sn = rtx[i].meta.ext_sn;
    o.ext_ts = rtx[i].meta.ext_ts;
    o.out_off = off[i];
    o.dt = uint32_t(rtx[i].dt);
    o.pkt = i;
    o.out_len = uint16_t(len[i]);
    o.flags = rtx[i].meta.marker ? LKF_OUT_MARKER : 0;
    o.layer = rtx[i].meta.layer;
  }
  return LKF_OK;
}

// Receiver.ReadRTP(layer, sourceSeqNo) (receiver.go:559-566) from the GPU
// buckets: the DownTrack's track buffer of the record's layer (an SVC track's
// single buffer; a closed buffer returns io.EOF), Bucket.GetPacket on the
// device, then the retransmissions as lkf_rtx_emit.
int lkf_rtx_emit_bucket(lkf_engine *e, const lkf_rtx *rtx, uint32_t n, lkf_out *out, uint8_t *out_arena,
                        uint64_t out_cap, uint32_t *n_out, uint64_t *out_len) {
  if (!e || !n_out || !out_len || (n && !rtx)) return LKF_EINVAL;
  *n_out = 0;
  *out_len = 0;
  if (!n) return LKF_OK;
  STEP(check_handles(&rtx[0].dt, sizeof(*rtx), n, e->dtp.size(), {}));
  Frame f(e, Order::BehindSender);
  STEP(rtx_open(f, n));
  std::vector<int32_t> sid(n, -1);
  std::vector<uint16_t> sn(n);
  {
    std::vector<std::vector<int32_t>> byTrack(e->tracks.size());
    for (size_t s = 0; s < e->streams.size(); s++) byTrack[size_t(e->streams[s].track)].push_back(int32_t(s));
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t t = e->dtp[size_t(rtx[i].dt)].track;
      sn[i] = rtx[i].meta.source_sn;
      if (!e->trackActive[t]) continue;
      const auto &v = byTrack[t];
      const int layer = rtx[i].meta.layer < 0 ? 0 : rtx[i].meta.layer;
      if (v.size() == 1) {
        sid[i] = v[0];
      } else {
        for (int32_t s : v)
          if (e->streams[size_t(s)].layer == layer) sid[i] = s;
      }
    }
  }
  if (!e->bktSlots) std::fill(sid.begin(), sid.end(), -1);
  STEP(f.grow("alloc bucket reads", want(e->dBktStream, n, 1024), want(e->dBktSn, n, 1024)));
  // (uploads on the sender stream, ahead of k_bkt_read / k_rtx: see lkf_rtx_emit)
  STEP(f.up(e->dRtx, rtx, n * sizeof(lkf_rtx), "rtx copy"));
  STEP(f.up(e->dBktStream, sid.data(), n * sizeof(int32_t), "bucket read copy"));
  STEP(f.up(e->dBktSn, sn.data(), n * sizeof(uint16_t), "bucket sn copy"));
  HIPCHK(e->dRtxIn.reserve(uint64_t(n) * kBktSlot + 64, 1 << 20), "alloc rtx in");  // (the queued uploads do not touch it)
  HIPCHK(launch_bucket_read(e->sendS, n, e->dBktStream, e->dBktSn, e->dBkt, e->dBktTag, e->dBktRing, e->dRtxIn,
                            e->dRtxSrc),
         "bucket read");
  std::vector<lkf_raw_pkt> src(n);
  STEP(f.down(src.data(), e->dRtxSrc, n * sizeof(lkf_raw_pkt), "src back"));
  STEP(f.wait());
  std::vector<uint16_t> hdr(n, 0);
  for (uint32_t i = 0; i < n; i++) hdr[i] = uint16_t(src[i].len ? src[i].reserved : 0);
  return rtx_emit_common(f, rtx, n, e->dRtxIn, hdr, out, out_arena, out_cap, n_out, out_len);
}

// ---- padding / blank frames (downtrack.go:764-859, :1307-1401) -------------
// Worst-case space per request is reserved (padding: ceil(bytes / 275)
// packets of at most 12 + 8 + 255 bytes; blank: two packets of at most
// 12 + 8 + 80), the kernel fills what it sends, the host packs it.
// sendingPacket -> RTPStatsSender.Update for host-listed packets (padding,
// blank frames, RTX): grouped by DownTrack in call order, one thread per
// DownTrack (k_sender_updates).  Runs on the sender stream, after the queued
// runs' sender statistics (sender or emit stream), which update the same
// DownTracks' RTPStatsSender, and after the producing kernel (the caller has
// waited for it).
static int sender_list(lkf_engine *e, std::vector<SenderUpd> &list) {
  if (list.empty()) return LKF_OK;
  std::stable_sort(list.begin(), list.end(), [](const SenderUpd &a, const SenderUpd &b) { return a.dt < b.dt; });
  std::vector<uint32_t> g;
  STEP(check_handles(&list[0].dt, sizeof(SenderUpd), uint32_t(list.size()), e->dtp.size(), {Repeat::Groups, &g, true}));
  Frame f(e, Order::BehindSender);
  STEP(f.open(false));
  STEP(f.grow("alloc sender list", want(e->dSSList, list.size(), 4096, 2 * list.size()),
              want(e->dSSGroups, g.size(), 4097, 2 * list.size() + 1)));
  STEP(f.up(e->dSSList, list.data(), list.size() * sizeof(SenderUpd), "sender list copy"));
  STEP(f.up(e->dSSGroups, g.data(), g.size() * sizeof(uint32_t), "sender groups copy"));
  SenderListLaunch a;
  a.list = e->dSSList;
  a.gBegin = e->dSSGroups;
  a.ngroups = uint32_t(g.size() - 1);
  a.ss = e->dSS;
  a.ring = e->dSSRing;
  a.gap = e->dSSGap;
  HIPCHK(launch_sender_updates(f.s, a), "sender updates");
  return f.wait();
}

// a padding / blank packet's header with the pacer's extension block
// (abs-send-time) and the TWCC interceptor's element (k_pad pad_hdr_len)
static uint32_t pad_hdr_bytes(const lkf_downtrack_params &p) {
  const uint32_t eb = (p.ext_abs_send_time ? 4u : 0u) + (p.ext_transport_cc ? 3u : 0u);
  return eb ? 16u + ((eb + 3) & ~3u) : 12u;
}

static int pad_common(lkf_engine *e, int blank, const lkf_pad_req *reqs, uint32_t n, int64_t now_ns, lkf_out *out,
                      uint8_t *arena, uint64_t out_cap, uint64_t arena_cap, uint32_t *n_out, uint64_t *arena_len,
                      uint32_t *bytes_sent) {
  if (!e || !n_out || !arena_len || (n && !reqs)) return LKF_EINVAL;
  *n_out = 0;
  *arena_len = 0;
  if (!n) return LKF_OK;
  STEP(check_handles(&reqs[0].dt, sizeof(*reqs), n, e->dtp.size(), {Repeat::DistinctEinval}));
  std::vector<uint64_t> off(2 * size_t(n));
  uint64_t recs = 0, bytes = 0;
  for (uint32_t i = 0; i < n; i++) {
    const int32_t dt = reqs[i].dt;
    const uint64_t np = !e->active[dt] ? 0 : blank ? 2 : (uint64_t(reqs[i].bytes_to_send) + 274) / 275;
    off[i] = recs;
    off[n + i] = bytes;
    recs += np;
    bytes += np * (blank ? 112 : 288);
  }
  // k_pad reads and writes the DownTracks' Forwarder / sequencer state, which
  // between runs only the decide stream touches: it runs there, behind the
  // queued decides (their emits keep running); its sendingPacket updates go to
  // the sender stream (sender_list)
  Frame f(e, Order::BehindDecide);
  STEP(f.open(true, true));
  const hipStream_t ds = f.s;
  STEP(f.grow("alloc pad requests", want(e->dPadReq, n, 1024), want(e->dPadOff, 2 * uint64_t(n), 2048),
              want(e->dPadCnt, 2 * uint64_t(n), 2048)));
  STEP(f.grow("alloc pad out", want(e->dPadOut, recs, 4096), want(e->dPadArena, bytes, 1 << 20)));
  // a removed DownTrack sends nothing: its request is dropped before the kernel
  std::vector<lkf_pad_req> q(reqs, reqs + n);
  std::vector<uint32_t> live;
  for (uint32_t i = 0; i < n; i++)
    if (e->active[q[i].dt]) live.push_back(i);
  std::vector<lkf_pad_req> lq(live.size());
  std::vector<uint64_t> loff(2 * live.size());
  for (size_t j = 0; j < live.size(); j++) {
    lq[j] = q[live[j]];
    loff[j] = off[live[j]];
    loff[live.size() + j] = off[n + live[j]];
  }
  const uint32_t m = uint32_t(live.size());
  std::vector<uint32_t> cnt(2 * size_t(m), 0);
  if (m) {
    // the request uploads on the decide stream, ordered ahead of k_pad (see lkf_rtx_emit)
    STEP(f.up(e->dPadReq, lq.data(), m * sizeof(lkf_pad_req), "pad req copy"));
    STEP(f.up(e->dPadOff, loff.data(), 2 * size_t(m) * sizeof(uint64_t), "pad off copy"));
    PadArgs a{};
    a.blank = blank;
    a.n = m;
    a.reqs = e->dPadReq;
    a.nowNs = now_ns;
    a.hot = e->dHot;
    a.dts = e->dDTs;
    a.tracks = e->dTracks;
    a.rm = e->dRm;
    a.seq = e->dSeq;
    a.seqSize = e->cfg.seq_size;
    a.srm = e->dSrm;
    a.srmStride = e->srmStride;
    a.srmCap = e->srmCap;
    a.dtCum = e->dDTCum;
    a.recOff = e->dPadOff;
    a.byteOff = e->dPadOff + m;
    a.out = e->dPadOut;
    a.arena = e->dPadArena;
    a.cnt = e->dPadCnt;
    a.bytes = e->dPadCnt + m;
    HIPCHK(launch_pad(ds, a), "pad");
    if (e->anyTwcc)  // transport-cc numbers in request (send) order
      HIPCHK(launch_twcc_stamp(ds, e->dDTs, e->dTwccCtrD, e->dTwccCtrT, m, e->dPadOut, e->dPadOff, e->dPadCnt, nullptr,
                               nullptr, nullptr, e->dPadArena),
             "twcc stamp");
    STEP(f.wait());
    D2H(cnt.data(), e->dPadCnt, 2 * size_t(m) * sizeof(uint32_t), "pad cnt copy");
  }
  if (bytes_sent)
    for (uint32_t i = 0; i < n; i++) bytes_sent[i] = 0;
  uint64_t k = 0, tot = 0;
  for (uint32_t j = 0; j < m; j++) {
    k += cnt[j];
    if (bytes_sent) bytes_sent[live[j]] = cnt[m + j];
    if (!blank && cnt[j] && !e->seqRM[lq[j].dt]) {  // pushPadding ran: reschedule (rebuild_sched)
      e->seqRM[lq[j].dt] = 1;
      e->schedDirty = true;
    }
  }
  std::vector<lkf_out> recv(recs ? recs : 1);
  std::vector<uint8_t> arv(bytes ? bytes : 1);
  if (k) {
    D2H(recv.data(), e->dPadOut, recs * sizeof(lkf_out), "pad out copy");
    D2H(arv.data(), e->dPadArena, bytes, "pad arena copy");
    // sendingPacket (downtrack.go:835-846, :1377-1386): isPadding, a 12-B
    // header (the pacer adds the extensions later), the payload as padding
    std::vector<SenderUpd> ul;
    for (uint32_t j = 0; j < m; j++)
      for (uint32_t c = 0; c < cnt[j]; c++) {
        const lkf_out &o = recv[loff[j] + c];
        SenderUpd u;
        std::memset(&u, 0, sizeof(u));
        u.esn = o.ext_sn;
        u.ets = o.ext_ts;
        u.t = now_ns;
        u.dt = o.dt;
        u.hdr = 12;
        u.pay = 0;
        u.pad = uint16_t(o.out_len - pad_hdr_bytes(e->dtp[o.dt]));
        u.marker = (o.flags & LKF_OUT_MARKER) ? 1 : 0;
        ul.push_back(u);
      }
    STEP(sender_list(e, ul));
  }
  for (uint32_t j = 0; j < m; j++)
    for (uint32_t c = 0; c < cnt[j]; c++) tot += (uint64_t(recv[loff[j] + c].out_len) + 15) & ~uint64_t(15);
  *n_out = uint32_t(k);
  *arena_len = tot;
  if (k > out_cap || tot > arena_cap || (k && (!out || !arena))) return LKF_ENOSPC;
  uint64_t w = 0, pos = 0;
  for (uint32_t j = 0; j < m; j++)
    for (uint32_t c = 0; c < cnt[j]; c++) {
      lkf_out o = recv[loff[j] + c];
      const uint64_t al = (uint64_t(o.out_len) + 15) & ~uint64_t(15);
      std::memcpy(arena + pos, arv.data() + o.out_off, al);
      o.out_off = pos;
      o.pkt = live[j];
      out[w++] = o;
      pos += al;
    }
  return LKF_OK;
}

// ---- the dependency-descriptor stream tracker (streamtracker_dd.go) --------
int32_t lkf_add_stream_tracker_dd(lkf_engine *e, int32_t track) {
  if (!e || track < 0 || track >= int32_t(e->tracks.size()) || !track_has_dd(e->tracks[track])) return LKF_EINVAL;
  if (e->trackDDTrk.size() < e->tracks.size()) e->trackDDTrk.resize(e->tracks.size(), -1);
  if (e->trackDDTrk[track] >= 0) return LKF_EINVAL;
  STEP(quiesce(e));
  if (!e->dTrackDDTrk) {
    HIPCHK(e->dTrackDDTrk.alloc(e->cfg.max_tracks), "alloc track dd trackers");
    HIPCHK(hipMemset(e->dTrackDDTrk, 0xff, size_t(e->cfg.max_tracks) * sizeof(uint32_t)), "track dd trackers reset");
  }
  if (e->nDDTrk + 1 > e->dDDTrk.cap()) {  // grow, keeping the trackers
    DevBuf<DDTrkState> n;
    HIPCHK(n.alloc(std::max<uint32_t>(2 * uint32_t(e->dDDTrk.cap()), 256)), "alloc dd trackers");
    if (e->nDDTrk) HIPCHK(hipMemcpy(n, e->dDDTrk, e->nDDTrk * sizeof(DDTrkState), hipMemcpyDeviceToDevice), "dd trackers move");
    e->dDDTrk = std::move(n);
  }
  DDTrkState t;
  std::memset(&t, 0, sizeof(t));
  t.maxS = t.maxT = -1;
  for (int l = 0; l < 3; l++) t.lastNotified[l] = -1;
  t.track = uint32_t(track);
  const uint32_t id = e->nDDTrk++;
  HIPCHK(hipMemcpy(e->dDDTrk + id, &t, sizeof(t), hipMemcpyHostToDevice), "dd tracker init");
  HIPCHK(hipMemcpy(e->dTrackDDTrk + track, &id, sizeof(id), hipMemcpyHostToDevice), "track dd tracker");
  e->trackDDTrk[track] = int32_t(id);
  e->epoch++;  // the prep graph's k_dd_decode observes the trackers
  return upload_done(e) ? LKF_EHIP : int32_t(id);
}

// SetPaused / Stop (streamtracker_dd.go:57-68, :123-137) on the host copy
int lkf_dd_tracker_ctl(lkf_engine *e, int32_t tracker, int32_t op, int32_t arg) {
  if (!e || tracker < 0 || uint32_t(tracker) >= e->nDDTrk) return LKF_EINVAL;
  if (op != LKF_TRACKER_PAUSE && op != LKF_TRACKER_STOP) return LKF_EINVAL;
  STEP(quiesce(e, false));
  DDTrkState t;
  D2H(&t, e->dDDTrk + tracker, sizeof(t), "dd tracker read");
  if (op == LKF_TRACKER_STOP) {
    if (!(t.flags & DT_STOPPED)) t.flags = (t.flags | DT_STOPPED) & ~DT_WORKER;
  } else {
    const bool p = arg != 0;
    if (bool(t.flags & DT_PAUSED) != p) {
      if (p) {
        t.flags |= DT_PAUSED | DT_WORKER;  // a worker drains the bitrates while paused
      } else {  // resetLocked :108-121
        t.flags &= ~(DT_PAUSED | DT_WORKER);
        std::memset(t.bytes, 0, sizeof(t.bytes));
        std::memset(t.bitrate, 0, sizeof(t.bitrate));
      }
    }
  }
  return write_row(e, e->dDDTrk + tracker, t, "dd tracker write");
}

int lkf_dd_trackers_tick(lkf_engine *e, const int32_t *trackers, uint32_t n, int64_t bitrate_elapsed_ns,
                         lkf_dd_tracker_status *out) {
  if (!e || (n && (!trackers || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  STEP(check_handles(trackers, sizeof(*trackers), n, e->nDDTrk, {Repeat::DistinctEinval}));
  Frame f(e, Order::Quiesced);
  STEP(f.open(false));
  STEP(f.grow("alloc dd tracker scratch", want(e->dDDTrkIds, n, 1024), want(e->dDDTrkOut, n, 1024)));
  STEP(f.up(e->dDDTrkIds, trackers, n * sizeof(int32_t), "dd tracker ids copy"));
  STEP(f.uploaded());
  HIPCHK(launch_dd_tracker_tick(f.s, e->dDDTrk, e->dDDTrkIds, n, bitrate_elapsed_ns, e->dDDTrkOut), "dd tracker tick");
  STEP(f.wait());
  D2H(out, e->dDDTrkOut, n * sizeof(lkf_dd_tracker_status), "dd tracker out copy");
  return LKF_OK;
}

// ---- stream trackers (streamtracker.go, streamtracker_packet.go) ------------
int32_t lkf_add_stream_tracker(lkf_engine *e, int32_t track, int32_t layer, uint32_t samples_required,
                               uint32_t cycles_required) {
  if (!e || track < 0 || track >= int32_t(e->tracks.size()) || layer < 0) return LKF_EINVAL;
  STEP(quiesce(e, false));
  if (e->nTrk + 1 > e->dTrk.cap()) {  // grow, keeping the trackers
    DevBuf<TrackerState> n;
    HIPCHK(n.alloc(std::max<uint32_t>(2 * uint32_t(e->dTrk.cap()), 1024)), "alloc trackers");
    if (e->nTrk) HIPCHK(hipMemcpy(n, e->dTrk, e->nTrk * sizeof(TrackerState), hipMemcpyDeviceToDevice), "trackers move");
    e->dTrk = std::move(n);
  }
  e->epoch++;  // the prep graph observes every tracker
  TrackerState t = {};
  t.track = uint32_t(track);
  t.layer = layer;
  t.samples = samples_required;
  t.cycles = cycles_required;
  STEP(write_row(e, e->dTrk + e->nTrk, t, "tracker init"));
  return int32_t(e->nTrk++);
}

// a StreamTrackerFrame (streamtracker_frame.go:39-211) with the source's
// StreamTrackerFrameConfig.MinFPS (config.go:413-458)
int32_t lkf_add_stream_tracker_frame(lkf_engine *e, int32_t track, int32_t layer, uint32_t clock_rate,
                                     double min_fps) {
  if (!e || track < 0 || track >= int32_t(e->tracks.size()) || layer < 0 || clock_rate == 0) return LKF_EINVAL;
  const int32_t id = lkf_add_stream_tracker(e, track, layer, 0, 0);
  if (id < 0) return id;
  TrackerState t;
  D2H(&t, e->dTrk + id, sizeof(t), "tracker read");
  t.frame = 1;
  t.clockRate = clock_rate;
  t.minFPS = min_fps;
  tracker_frame_reset_fps(t);
  const int rc = write_row(e, e->dTrk + id, t, "tracker write");
  return rc ? rc : id;
}

// Reset / SetPaused / Stop (streamtracker.go:127-185) on the host copy of the state
int lkf_stream_tracker_ctl(lkf_engine *e, int32_t tracker, int32_t op, int32_t arg) {
  if (!e || tracker < 0 || uint32_t(tracker) >= e->nTrk) return LKF_EINVAL;
  STEP(quiesce(e, false));
  TrackerState t;
  D2H(&t, e->dTrk + tracker, sizeof(t), "tracker read");
  auto resetLocked = [&]() {
    t.workerLive = 0;  // generation bump: the worker exits
    t.status = 0;
    for (int i = 0; i < 4; i++) t.bytes[i] = t.bitrate[i] = 0;
    t.countSinceLast = t.cycleCount = 0;
    t.initialized = 0;
    if (t.frame) {  // StreamTrackerFrame.Reset
      tracker_frame_reset_fps(t);
      t.lastCheckSet = 0;
      t.lastCheckNs = 0;
    }
  };
  auto notify = [&]() {
    if (t.status != t.lastNotified) {
      t.lastNotified = t.status;
      t.notifications++;
    }
  };
  switch (op) {
    case LKF_TRACKER_RESET:
      if (t.stopped) return LKF_OK;
      resetLocked();
      notify();
      break;
    case LKF_TRACKER_PAUSE:
      t.paused = arg != 0;
      if (!t.paused) {
        resetLocked();
      } else {
        t.workerLive = 0;
        t.status = 0;
      }
      notify();
      break;
    case LKF_TRACKER_STOP:
      if (t.stopped) return LKF_OK;
      t.stopped = 1;
      t.workerLive = 0;
      break;
    default:
      return LKF_EINVAL;
  }
  return write_row(e, e->dTrk + tracker, t, "tracker write");
}

int lkf_stream_trackers_tick(lkf_engine *e, const int32_t *trackers, uint32_t n, int check, int64_t bitrate_elapsed_ns,
                             lkf_tracker_status *out) {
  return lkf_stream_trackers_tick_at(e, trackers, n, check, bitrate_elapsed_ns, 0, out);
}
int lkf_stream_trackers_tick_at(lkf_engine *e, const int32_t *trackers, uint32_t n, int check,
                                int64_t bitrate_elapsed_ns, int64_t now_ns, lkf_tracker_status *out) {
  if (!e || (n && (!trackers || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  STEP(check_handles(trackers, sizeof(*trackers), n, e->nTrk, {Repeat::DistinctEinval}));
  Frame f(e, Order::Quiesced);
  STEP(f.open(false));
  STEP(f.grow("alloc tracker scratch", want(e->dTrkIds, n, 1024), want(e->dTrkOut, n, 1024)));
  STEP(f.up(e->dTrkIds, trackers, n * sizeof(int32_t), "tracker ids copy"));
  STEP(f.uploaded());
  HIPCHK(launch_tracker_tick(f.s, e->dTrk, e->dTrkIds, n, check, bitrate_elapsed_ns, now_ns, e->dTrkOut), "tracker tick");
  STEP(f.wait());
  D2H(out, e->dTrkOut, n * sizeof(lkf_tracker_status), "tracker out copy");
  return LKF_OK;
}

// ---- RED for Opus (redreceiver.go, redprimaryreceiver.go) -------------------
static int red_common(lkf_engine *e, bool decode, const lkf_pkt *pkts, uint32_t n, const uint8_t *arena,
                      uint64_t arena_len, const int32_t *map, uint32_t map_len, lkf_pkt *out, uint32_t out_cap,
                      uint8_t *out_arena, uint64_t out_arena_cap, uint32_t *n_out, uint64_t *out_arena_len) {
  if (!e || !n_out || !out_arena_len || (n && (!pkts || !arena)) || (map_len && !map)) return LKF_EINVAL;
  *n_out = 0;
  *out_arena_len = 0;
  const uint32_t nt = uint32_t(e->tracks.size());
  if (map_len > nt) return LKF_EINVAL;
  for (uint32_t t = 0; t < map_len; t++)
    if (map[t] >= int32_t(nt) || map[t] < -1) return LKF_EINVAL;
  // groups: the mapped tracks' contiguous packet runs (each track once)
  std::vector<uint32_t> gb, ge;
  std::vector<uint8_t> seen(nt, 0);
  std::vector<uint64_t> off(2 * size_t(n) + 1, 0);
  uint64_t recs = 0, bytes = 0;
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t t = pkts[i].track;
    if (t >= nt || uint64_t(pkts[i].arena_off) + pkts[i].payload_off + pkts[i].payload_len > arena_len)
      return LKF_EINVAL;
    if (i == 0 || pkts[i - 1].track != t) {
      if (seen[t]) return LKF_EORDER;
      seen[t] = 1;
      if (t < map_len && map[t] >= 0) {
        gb.push_back(i);
        ge.push_back(i);
      }
    }
    const bool mapped = t < map_len && map[t] >= 0;
    if (mapped) ge.back() = i + 1;
    off[i] = recs;
    off[n + i] = bytes;
    if (mapped) {
      const uint64_t hdr = pkts[i].payload_off, pl = pkts[i].payload_len;
      recs += decode ? 3 : 1;
      bytes += decode ? 3 * ((hdr + pl + 15) & ~15ull) : ((hdr + std::max<uint64_t>(1500, pl + 1) + 15) & ~15ull);
    }
  }
  Frame f(e, Order::Quiesced);
  STEP(f.open());
  if (!gb.empty()) {
    auto &r = e->red;
    if (decode && !e->dRedDec) {
      HIPCHK(e->dRedDec.alloc(e->cfg.max_tracks), "alloc red dec");
      HIPCHK(hipMemset(e->dRedDec, 0, size_t(e->cfg.max_tracks) * sizeof(RedDecState)), "red dec reset");
    }
    if (!decode && !e->dRedEnc) {
      HIPCHK(e->dRedEnc.alloc(e->cfg.max_tracks), "alloc red enc");
      HIPCHK(hipMemset(e->dRedEnc, 0, size_t(e->cfg.max_tracks) * sizeof(RedEncState)), "red enc reset");
    }
    STEP(f.grow("alloc red scratch", want(r.in, n, 1024), want(r.inArena, arena_len + 64, 1024),
                want(r.out, recs, 1024), want(r.outArena, bytes, 1024), want(r.g, 2 * gb.size(), 1024),
                want(r.cnt, n, 1024), want(r.map, nt, 1024), want(r.off, 2 * uint64_t(n) + 1, 1024)));
    std::vector<int32_t> mp(nt, -1);
    for (uint32_t t = 0; t < map_len; t++) mp[t] = map[t];
    std::vector<uint32_t> g(gb);
    g.insert(g.end(), ge.begin(), ge.end());
    STEP(f.up(r.in, pkts, n * sizeof(lkf_pkt), "red in copy"));
    STEP(f.up(r.inArena, arena, arena_len, "red arena copy"));
    STEP(f.up(r.g, g.data(), g.size() * sizeof(uint32_t), "red groups copy"));
    STEP(f.up(r.map, mp.data(), nt * sizeof(int32_t), "red map copy"));
    STEP(f.up(r.off, off.data(), 2 * size_t(n) * sizeof(uint64_t), "red off copy"));
    HIPCHK(hipMemset(r.cnt, 0, n * sizeof(uint32_t)), "red counts reset");
    STEP(f.uploaded());
    RedLaunch a;
    a.in = r.in;
    a.inArena = r.inArena;
    a.gBegin = r.g;
    a.gEnd = r.g + gb.size();
    a.ngroups = uint32_t(gb.size());
    a.map = r.map;
    a.enc = e->dRedEnc;
    a.dec = e->dRedDec;
    a.recOff = r.off;
    a.byteOff = r.off + n;
    a.out = r.out;
    a.outArena = r.outArena;
    a.cnt = r.cnt;
    HIPCHK(launch_red(f.s, decode, a), "red");
    STEP(f.wait());
  }
  std::vector<uint32_t> cnt(n, 0);
  std::vector<lkf_pkt> rec(recs ? recs : 1);
  std::vector<uint8_t> ar(bytes ? bytes : 1);
  if (!gb.empty()) {
    D2H(cnt.data(), e->red.cnt, n * sizeof(uint32_t), "red cnt copy");
    if (recs) D2H(rec.data(), e->red.out, recs * sizeof(lkf_pkt), "red out copy");
    if (bytes) D2H(ar.data(), e->red.outArena, bytes, "red arena copy");
  }
  uint64_t k = 0, tot = 0;
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t c = 0; c < cnt[i]; c++) {
      const lkf_pkt &o = rec[off[i] + c];
      tot += (uint64_t(o.payload_off) + o.payload_len + 15) & ~15ull;
      k++;
    }
  *n_out = uint32_t(k);
  *out_arena_len = tot;
  if (k > out_cap || tot > out_arena_cap || (k && (!out || !out_arena))) return LKF_ENOSPC;
  uint64_t w = 0, pos = 0;
  for (uint32_t i = 0; i < n; i++)
    for (uint32_t c = 0; c < cnt[i]; c++) {
      lkf_pkt o = rec[off[i] + c];
      const uint64_t len = uint64_t(o.payload_off) + o.payload_len, al = (len + 15) & ~15ull;
      std::memcpy(out_arena + pos, ar.data() + o.arena_off, len);
      std::memset(out_arena + pos + len, 0, al - len);
      o.arena_off = uint32_t(pos);
      out[w++] = o;
      pos += al;
    }
  return LKF_OK;
}

int lkf_red_encode(lkf_engine *e, const lkf_pkt *pkts, uint32_t n, const uint8_t *arena, uint64_t arena_len,
                   const int32_t *map, uint32_t map_len, lkf_pkt *out, uint32_t out_cap, uint8_t *out_arena,
                   uint64_t out_arena_cap, uint32_t *n_out, uint64_t *out_arena_len) {
  return red_common(e, false, pkts, n, arena, arena_len, map, map_len, out, out_cap, out_arena, out_arena_cap, n_out,
                    out_arena_len);
}
int lkf_red_decode(lkf_engine *e, const lkf_pkt *pkts, uint32_t n, const uint8_t *arena, uint64_t arena_len,
                   const int32_t *map, uint32_t map_len, lkf_pkt *out, uint32_t out_cap, uint8_t *out_arena,
                   uint64_t out_arena_cap, uint32_t *n_out, uint64_t *out_arena_len) {
  return red_common(e, true, pkts, n, arena, arena_len, map, map_len, out, out_cap, out_arena, out_arena_cap, n_out,
                    out_arena_len);
}

// ---- Forwarder allocation: AllocateOptimal (forwarder.go:591-725),
// AllocateNextHigher (:1107-1217), GetNextHigherTransition (:1219-1306),
// Pause (:1308-1351) ------------------------------------------------------
// The allocation calls' three buffers grow together, dAllocCapacity last (its
// capacity is what all of them hold; 0 after a failed grow); likewise the
// provisional pass's request and result buffers, dProvOut (bytes) last.
static uint64_t alloc_cap(const lkf_engine *e) { return e->dAllocCapacity.cap(); }
static int alloc_grow(Frame &f, uint32_t n) {
  lkf_engine *e = f.e;
  return f.grow("alloc allocation scratch", want(e->dAllocReq, n, 1024), want(e->dAllocOut, n, 1024),
                want(e->dAllocCapacity, n, 1024));
}
static int alloc_common(lkf_engine *e, int mode, const lkf_alloc_req *reqs, const int64_t *capacity, uint32_t n,
                        void *out, size_t outSize) {
  if (!e || (n && (!reqs || !out || (mode == ALLOC_NEXT_HIGHER && !capacity)))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  HandleFault why;  // a removed DownTrack has no allocation (its state stays as it was)
  const HandlePolicy p{Repeat::DistinctEinval, nullptr, false, e->active.data(), Inactive::Refuse, &why};
  if (const int rc = check_handles(&reqs[0].dt, sizeof(*reqs), n, e->dtp.size(), p)) {
    if (why == HandleFault::Inactive) e->err = "allocation request for a removed DownTrack";
    return rc;
  }
  // The allocation reads and writes the DownTracks' hot state and last
  // allocation, which between runs only the decide stream touches: it is
  // ordered on that stream after the queued runs' decides (Order::BehindDecide),
  // and the host waits for it alone, not for their emits, sender statistics or
  // protect stages (those keep overlapping the call).
  Frame f(e, Order::BehindDecide);
  STEP(f.open());
  STEP(alloc_grow(f, n));
  static_assert(sizeof(lkf_video_transition) <= sizeof(lkf_allocation), "transition fits the out buffer");
  STEP(f.up(e->dAllocReq, reqs, n * sizeof(lkf_alloc_req), "alloc req copy"));
  if (mode == ALLOC_NEXT_HIGHER) STEP(f.up(e->dAllocCapacity, capacity, n * sizeof(int64_t), "capacity copy"));
  HIPCHK(launch_allocate(f.s, mode, e->dAllocReq, e->dAllocCapacity, n, e->dHot, e->dDTs, e->dTracks, e->dLastAlloc,
                         e->dAllocOut),
         "allocate");
  STEP(f.down(out, e->dAllocOut, n * outSize, "alloc out copy"));
  return f.wait();
}
int lkf_allocate_optimal(lkf_engine *e, const lkf_alloc_req *reqs, uint32_t n, lkf_allocation *out) {
  return alloc_common(e, ALLOC_OPTIMAL, reqs, nullptr, n, out, sizeof(lkf_allocation));
}
int lkf_allocate_next_higher(lkf_engine *e, const lkf_alloc_req *reqs, const int64_t *capacity, uint32_t n,
                             lkf_allocation *out) {
  return alloc_common(e, ALLOC_NEXT_HIGHER, reqs, capacity, n, out, sizeof(lkf_allocation));
}
int lkf_next_higher_transition(lkf_engine *e, const lkf_alloc_req *reqs, uint32_t n, lkf_video_transition *out) {
  return alloc_common(e, ALLOC_TRANSITION, reqs, nullptr, n, out, sizeof(lkf_video_transition));
}
int lkf_pause(lkf_engine *e, const lkf_alloc_req *reqs, uint32_t n, lkf_allocation *out) {
  return alloc_common(e, ALLOC_PAUSE, reqs, nullptr, n, out, sizeof(lkf_allocation));
}

// ---- the cooperative allocation pass (Provisional*, allocateAllTracks) ------
// distinct, active, video DownTracks (the reference's selector is nil for audio)
static int prov_check(lkf_engine *e, const int32_t *dts, uint32_t n, size_t stride) {
  const HandlePolicy p{Repeat::DistinctEinval, nullptr, false, e->active.data()};
  const int rc = check_handles(dts, stride, n, e->dtp.size(), p, [&](uint32_t i) {
    int32_t dt;
    std::memcpy(&dt, reinterpret_cast<const uint8_t *>(dts) + i * stride, sizeof(dt));
    return e->tracks[e->dtp[dt].track].kind == LKF_KIND_VIDEO;
  });
  if (rc) e->err = "provisional allocation: DownTracks must be distinct, active and video";
  return rc;
}
// The provisional pass's request and result buffers and the allocation calls'
// three (at least as large, and never shrunk) are one family here.
static int prov_grow(Frame &f, uint32_t n, uint32_t ngroups) {
  lkf_engine *e = f.e;
  const lkf_cfg &c = e->cfg;
  if (!e->dProv) {
    HIPCHK(e->dProv.alloc(c.max_downtracks), "alloc provisional");
    HIPCHK(hipMemset(e->dProv, 0, size_t(c.max_downtracks) * sizeof(ProvState)), "provisional reset");
  }
  const uint64_t ac = std::max<uint64_t>(alloc_cap(e), n);
  STEP(f.grow("alloc provisional scratch", want(e->dProvReq, n, 1024),
              want(e->dProvOut, n * sizeof(lkf_allocation), 1024 * sizeof(lkf_allocation)),
              want(e->dAllocReq, n, 1024, ac), want(e->dAllocOut, n, 1024, ac), want(e->dAllocCapacity, n, 1024, ac)));
  return f.grow("alloc prov groups", want(e->dProvGroups, ngroups, 256));
}
static int prov_common(lkf_engine *e, int mode, const lkf_prov_req *reqs, const lkf_alloc_req *alloc, uint32_t n,
                       void *out, size_t outSize) {
  if (!e || (n && !reqs && !alloc) || (n && outSize && !out)) return LKF_EINVAL;
  if (!n) return LKF_OK;
  STEP(alloc ? prov_check(e, &alloc[0].dt, n, sizeof(lkf_alloc_req)) : prov_check(e, &reqs[0].dt, n, sizeof(lkf_prov_req)));
  Frame f(e, Order::Quiesced);
  STEP(f.open());
  STEP(prov_grow(f, n, 0));
  if (alloc)
    STEP(f.up(e->dAllocReq, alloc, n * sizeof(lkf_alloc_req), "prov req copy"));
  else
    STEP(f.up(e->dProvReq, reqs, n * sizeof(lkf_prov_req), "prov req copy"));
  STEP(f.uploaded());
  ProvLaunch a;
  a.mode = mode;
  a.n = n;
  a.reqs = e->dProvReq;
  a.alloc = e->dAllocReq;
  a.hot = e->dHot;
  a.dts = e->dDTs;
  a.tracks = e->dTracks;
  a.last = e->dLastAlloc;
  a.prov = e->dProv;
  a.out = e->dProvOut;
  HIPCHK(launch_prov(f.s, a), "provisional");
  STEP(f.wait());
  if (outSize) D2H(out, e->dProvOut, n * outSize, "prov out copy");
  return LKF_OK;
}
static int prov_dts(lkf_engine *e, int mode, const int32_t *dts, uint32_t n, void *out, size_t outSize) {
  if (n && !dts) return LKF_EINVAL;
  std::vector<lkf_prov_req> r(n);
  for (uint32_t i = 0; i < n; i++) {
    std::memset(&r[i], 0, sizeof(r[i]));
    r[i].dt = dts[i];
  }
  return prov_common(e, mode, r.data(), nullptr, n, out, outSize);
}
int lkf_provisional_prepare(lkf_engine *e, const lkf_alloc_req *reqs, uint32_t n) {
  return prov_common(e, PROV_PREPARE, nullptr, reqs, n, nullptr, 0);
}
int lkf_provisional_reset(lkf_engine *e, const int32_t *dts, uint32_t n) {
  return prov_dts(e, PROV_RESET, dts, n, nullptr, 0);
}
int lkf_provisional_allocate(lkf_engine *e, const lkf_prov_req *reqs, uint32_t n, lkf_prov_result *out) {
  return prov_common(e, PROV_ALLOCATE, reqs, nullptr, n, out, sizeof(lkf_prov_result));
}
int lkf_provisional_cooperative(lkf_engine *e, const lkf_prov_req *reqs, uint32_t n, lkf_video_transition *out) {
  return prov_common(e, PROV_COOPERATIVE, reqs, nullptr, n, out, sizeof(lkf_video_transition));
}
int lkf_provisional_best_weighted(lkf_engine *e, const int32_t *dts, uint32_t n, lkf_video_transition *out) {
  return prov_dts(e, PROV_BEST_WEIGHTED, dts, n, out, sizeof(lkf_video_transition));
}
int lkf_provisional_commit(lkf_engine *e, const int32_t *dts, uint32_t n, lkf_allocation *out) {
  return prov_dts(e, PROV_COMMIT, dts, n, out, sizeof(lkf_allocation));
}
int lkf_allocate_all(lkf_engine *e, const lkf_alloc_group *groups, uint32_t ngroups, const lkf_alloc_req *reqs,
                     uint32_t n, lkf_allocation *out) {
  if (!e || (ngroups && !groups) || (n && (!reqs || !out))) return LKF_EINVAL;
  std::vector<uint8_t> cover(n, 0);  // groups are disjoint ranges of reqs
  for (uint32_t g = 0; g < ngroups; g++) {
    if (uint64_t(groups[g].first) + groups[g].count > n) return LKF_EINVAL;
    for (uint32_t k = 0; k < groups[g].count; k++)
      if (cover[groups[g].first + k]++) return LKF_EINVAL;
  }
  if (!ngroups || !n) return LKF_OK;
  STEP(prov_check(e, &reqs[0].dt, n, sizeof(lkf_alloc_req)));
  Frame f(e, Order::Quiesced);
  STEP(f.open());
  STEP(prov_grow(f, n, ngroups));
  STEP(f.up(e->dAllocReq, reqs, n * sizeof(lkf_alloc_req), "alloc req copy"));
  STEP(f.up(e->dProvGroups, groups, ngroups * sizeof(lkf_alloc_group), "groups copy"));
  HIPCHK(hipMemset(e->dProvOut, 0, n * sizeof(lkf_allocation)), "alloc out reset");
  STEP(f.uploaded());
  HIPCHK(launch_allocate_all(f.s, e->dProvGroups, ngroups, e->dAllocReq, e->dHot, e->dDTs, e->dTracks,
                             e->dLastAlloc, e->dProv, reinterpret_cast<lkf_allocation *>(e->dProvOut.get())),
         "allocate all");
  STEP(f.wait());
  D2H(out, e->dProvOut, n * sizeof(lkf_allocation), "alloc out copy");
  return LKF_OK;
}

int lkf_padding(lkf_engine *e, const lkf_pad_req *reqs, uint32_t n, int64_t now_ns, lkf_out *out, uint8_t *arena,
                uint64_t out_cap, uint64_t arena_cap, uint32_t *n_out, uint64_t *arena_len, uint32_t *bytes_sent) {
  return pad_common(e, 0, reqs, n, now_ns, out, arena, out_cap, arena_cap, n_out, arena_len, bytes_sent);
}

int lkf_blank_frames(lkf_engine *e, const lkf_pad_req *reqs, uint32_t n, int64_t now_ns, lkf_out *out, uint8_t *arena,
                     uint64_t out_cap, uint64_t arena_cap, uint32_t *n_out, uint64_t *arena_len) {
  return pad_common(e, 1, reqs, n, now_ns, out, arena, out_cap, arena_cap, n_out, arena_len, nullptr);
}

int lkf_last_timings(lkf_engine *e, float *decide_ms, float *emit_ms, float *total_ms) {
  return lkf_timing_window(e, 1, decide_ms, emit_ms, total_ms);
}

// decide = sum of the decide-kernel spans, emit = sum of the k_emit spans,
// total = GPU span from the first run's start to the last run's emit end
// (stages overlap across batches, so total < decide + emit).
int lkf_timing_window(lkf_engine *e, uint32_t n, float *decide_ms, float *emit_ms, float *total_ms) {
  if (!e || n == 0 || n > uint32_t(lkf_engine::kRing) || n > e->nRuns) return LKF_EINVAL;
  float sa = 0, sb = 0;
  const uint64_t first = e->nRuns - n;
  for (uint64_t r = first; r < e->nRuns; r++) {
    Event *rg = e->ring[r % lkf_engine::kRing];
    HIPCHK(hipEventSynchronize(rg[4]), "evsync");
    float a = 0, b = 0;
    HIPCHK(hipEventElapsedTime(&a, rg[1], rg[2]), "elapsed");
    HIPCHK(hipEventElapsedTime(&b, rg[3], rg[4]), "elapsed");
    sa += a;
    sb += b;
  }
  float c = 0;
  HIPCHK(hipEventElapsedTime(&c, e->ring[first % lkf_engine::kRing][0],
                             e->ring[(e->nRuns - 1) % lkf_engine::kRing][4]),
         "elapsed");
  if (decide_ms) *decide_ms = sa;
  if (emit_ms) *emit_ms = sb;
  if (total_ms) *total_ms = c;
  return LKF_OK;
}

// ---- ingress ------------------------------------------------------------------

// NewBuffer + Bind (buffer.go:124-215); AudioLevelParams defaults config.go:380-385.
int32_t lkf_add_stream(lkf_engine *e, const lkf_stream_params *p) {
  if (!e || !p || p->track < 0 || p->track >= int32_t(e->tracks.size())) return LKF_EINVAL;
  if (e->streams.size() >= e->maxStreams) return LKF_ENOSPC;
  const lkf_track_params &tp = e->tracks[p->track];
  DevStream d;
  std::memset(&d, 0, sizeof(d));
  d.track = uint32_t(p->track);
  d.layer = p->layer;
  d.ssrc = p->ssrc;
  d.clockRate = tp.clock_rate;
  d.codec = tp.codec;
  d.levelExt = p->audio_level_ext;
  d.ddExt = p->dd_ext;
  d.twccExt = p->twcc_ext;
  d.ddIdx = p->dd_ext ? e->nDDStreams++ : 0xffffffffu;  // its DependencyDescriptorParser (buffer.go:193-201)
  d.nack = p->nack ? 1 : 0;  // its NackQueue (buffer.go:248-256)
  const bool dflt = !p->active_level && !p->min_percentile && !p->observe_duration_ms && !p->smooth_intervals;
  d.activeLevel = dflt ? 35 : p->active_level;
  d.minPercentile = dflt ? 40 : p->min_percentile;
  d.observeDuration = dflt ? 400 : p->observe_duration_ms;
  const uint32_t smooth = dflt ? 2 : p->smooth_intervals;
  d.minActiveDuration = uint32_t(d.minPercentile) * d.observeDuration / 100;  // audiolevel.go:55
  d.smoothFactor = smooth > 0 ? double(2) / double(smooth + 1) : 1.0;
  d.activeThreshold = std::pow(10.0, double(d.activeLevel) * (-1.0 / 20));  // ConvertAudioLevel
  e->streams.push_back(*p);
  e->pendStreams.push_back(d);
  e->spkDirty = true;
  return int32_t(e->streams.size() - 1);
}

// Enqueued on the decide stream ahead of the batch's decide stage (no host
// sync): the ExtPacket count stays on the device (k_track_ranges reads it).
static int ingest_common(lkf_engine *e, BatchCtx &x, const lkf_raw_pkt *dRaws, uint32_t n, const uint8_t *dRaw,
                         uint64_t rawLen) {
  const uint32_t nt = uint32_t(e->tracks.size());
  hipStream_t s = e->ingS;
  // the batch's GPU span (lkf_timing_window total) starts before its ingest
  HIPCHK(hipEventRecord(e->ring[e->nRuns % lkf_engine::kRing][0], s), "event");
  e->ingestStarted = true;
  // this ingest's scratch set: the ingest two back used it, and its NACK
  // queues (side stream) and bucket copies (sender stream) read it
  const int par = e->ingPar ^ 1;
  e->ingPar = par;
  const lkf_engine::IngSet &g = e->ing[par];
  if (e->sidePending[par]) HIPCHK(hipStreamWaitEvent(s, e->sideDone[par], 0), "wait nack queues");
  e->sidePending[par] = false;
  if (e->bktPending[par]) HIPCHK(hipStreamWaitEvent(s, e->bktDone[par], 0), "wait bucket copies");
  e->bktPending[par] = false;
  // the previous run's resolver (datagram keys) still reads the scan this ingest overwrites
  if (e->scanReadPending) HIPCHK(hipStreamWaitEvent(s, e->scanRead, 0), "wait key resolve");
  e->scanReadPending = false;
  IngestLaunch a;
  a.raws = dRaws;
  a.n = n;
  a.raw = dRaw;
  a.streams = e->dStreams;
  a.nstreams = uint32_t(e->streams.size());
  a.ntracks = nt;
  a.hot = e->dStreamHot;
  a.hist = e->dHist;
  a.rxGap = e->dRxGap;
  a.rings = e->dStreamRings;
  a.parsed = g.parsed;
  a.tBegin = g.tBegin;
  a.tEnd = g.tEnd;
  a.tRuns = e->dITRuns;
  a.err = e->dIErr;
  a.flows = g.flows;
  a.fwd = g.fwd;
  a.twcc = e->dTwcc;
  a.pos = e->dPos;
  a.partA = e->dIPartA;
  a.partB = nullptr;
  a.total = x.dITotal;
  a.out = x.dPktsOwn;
  a.list = g.list;
  a.listCnt = g.listCnt;
  a.listStride = e->cfg.max_batch_pkts;
  a.nack = e->dNack;
  a.nackInfo = g.nackInfo;
  a.nackPairOff = g.nackPairOff;
  a.nackPairCnt = g.nackPairCnt;
  a.nackPairs = g.nackPairs;
  a.nackPairCap = e->nackPairCap;
  a.nackIn = g.nackIn;
  a.nackAlone = e->knobs.nackAlone;
  if (!e->fpsHandles.empty() || !e->fpsDDHandles.empty()) {  // (an empty ingest counts too: it completes nothing)
    a.nfps = uint32_t(e->fpsHandles.size());
    a.fpsList = e->dFpsList;
    a.fpsCalcAt = e->dFpsCalcAt;
    a.fpsStates = e->dFps;
    a.nfpsDD = uint32_t(e->fpsDDHandles.size());
    a.fpsDDList = e->dFpsDDList;
    a.fpsDDCalcAt = e->dFpsDDCalcAt;
    a.fpsDDStates = e->dFpsDD;
    a.fpsDDStructs = e->dFpsDDStruct;
    if (!++e->fpsEpoch) e->fpsEpoch = 1;  // (0 means "not yet" in dFpsCalcAt)
    a.fpsEpoch = e->fpsEpoch;
  }
  BucketLaunch bl;
  if (e->bktSlots && e->bktStorePending) {  // a second ingest before lkf_run: the first one's copies read this
                                            // context's store list first
    HIPCHK(hipEventRecord(e->bktEv, e->sendS), "event");
    HIPCHK(hipStreamWaitEvent(s, e->bktEv, 0), "wait bucket store");
  }
  if (e->bktSlots) {
    bl.raws = dRaws;
    bl.raw = dRaw;
    bl.n = n;
    bl.streams = e->dStreams;
    bl.nstreams = uint32_t(e->streams.size());
    bl.tBegin = g.tBegin;
    bl.tEnd = g.tEnd;
    bl.list = g.list;
    bl.listCnt = g.listCnt;
    bl.listStride = e->cfg.max_batch_pkts;
    bl.flows = g.flows;
    bl.fwd = g.fwd;
    bl.state = e->dBkt;
    bl.tag = e->dBktTag;
    bl.owner = e->dBktOwner;
    bl.store = x.dBktStore;
    bl.ring = e->dBktRing;
    bl.epoch = ++e->bktEpoch;
    a.bucket = &bl;
  }
  // the forwarding context's preparation for lkf_run (k_ing_out)
  a.fwdPrep.tBegin = x.dTBegin;
  a.fwdPrep.tEnd = x.dTEnd;
  a.fwdPrep.err = x.dErr;
  a.fwdPrep.fwdCnt = x.dFwdCnt;
  a.fwdPrep.stats = x.dStats;
  a.fwdPrep.fwdBytes = x.dFwdBytes;
  a.fwdPrep.nstats = kStatsWords * (1 + kStatCopies);
  a.fwdPrep.ndts = uint32_t(e->dtp.size());
  const bool dd = e->nDDStreams != 0;
  a.ddStates = dd ? e->dDDIng : nullptr;
  a.ddStructs = dd ? e->dDDIngStruct : nullptr;
  a.ingDD = dd ? e->dIngDD : nullptr;
  a.outDD = dd ? x.dDDIn : nullptr;
  {
    bool side = false;
    HIPCHK(launch_ingest(s, a, e->sideS, e->sideFork, e->sideDone[par], &side), "ingest");
    e->sidePending[par] = side;
  }
  if (a.bucket && n) {  // the bucket copies, off the forwarding path: the sender stream (the
                        // batch context counts as done only after it, like the sender statistics)
    HIPCHK(hipEventRecord(e->bktEv, s), "event");
    HIPCHK(hipStreamWaitEvent(e->sendS, e->bktEv, 0), "wait ingest (bucket store)");
    // (measurement only: LKF_SKIP_BKT_STORE=1 leaves the rings stale)
    if (!e->knobs.skipBktStore) HIPCHK(launch_bucket_store(e->sendS, bl), "bucket store");
    HIPCHK(hipEventRecord(e->bktDone[par], e->sendS), "event");
    e->bktPending[par] = true;
    e->bktStorePending = true;
  }
  HIPCHK(launch_err_fold(s, e->dIErr, e->dSticky, 8), "ingest error fold");
  HIPCHK(hipEventRecord(x.ingested, s), "event");  // the run's preparation (prep stream) waits for it
  x.fromIngest = true;
  x.prepByIngest = n != 0;
  x.prepNT = nt;
  x.prepND = uint32_t(e->dtp.size());
  e->lastIngestN = n;
  e->ingRaws = dRaws;
  e->curPkts = x.dPktsOwn;
  e->curN = n;  // launch bound; the count is x.dITotal
  // (an empty ingest launches nothing, so dITotal still holds an older
  // ingest's count: the batch is empty, with no device-side count)
  e->curNDev = n ? x.dITotal : nullptr;
  e->curFromIngest = true;
  e->curDD = a.outDD;  // the ExtPackets' descriptors (nullptr: no DD stream)
  e->curOwned = true;
  e->curDDOwned = true;
  e->curArena = dRaw;
  e->curArenaLen = rawLen;
  e->haveBatch = true;
  return LKF_OK;
}

// The ingest stream waits for what still reads the context's staging buffers
// (dRawPkts, dArenaOwn) before a host-form ingest overwrites them.
static int ingest_staging_waits(lkf_engine *e, BatchCtx &x) {
  if (x.used) HIPCHK(hipStreamWaitEvent(e->ingS, x.emitted, 0), "wait emit");  // batch n-3 reads these buffers
  if (e->haveBatch && e->curPkts == x.dPktsOwn) {
    // a second ingest into this context before lkf_run: the previous ingest's
    // NACK queues (side stream) and bucket copies (sender stream) still read
    // the datagrams these copies overwrite
    const int lp = e->ingPar;
    if (e->sidePending[lp]) HIPCHK(hipStreamWaitEvent(e->ingS, e->sideDone[lp], 0), "wait nack queues");
    if (e->bktPending[lp]) HIPCHK(hipStreamWaitEvent(e->ingS, e->bktDone[lp], 0), "wait bucket copies");
  }
  return LKF_OK;
}

int lkf_ingest(lkf_engine *e, const lkf_raw_pkt *pkts, uint32_t n, const uint8_t *raw, uint64_t raw_len) {
  if (!e || (n && (!pkts || !raw))) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts || raw_len > e->cfg.max_batch_arena) return LKF_ENOSPC;
  int rc = flush_topology(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[e->nRuns % lkf_engine::kCtx];
  rc = ingest_staging_waits(e, x);
  if (rc) return rc;
  if (n) HIPCHK(hipMemcpyAsync(x.dRawPkts, pkts, size_t(n) * sizeof(lkf_raw_pkt), hipMemcpyHostToDevice, e->ingS),
                "raw pkts");
  if (raw_len) HIPCHK(hipMemcpyAsync(x.dArenaOwn, raw, raw_len, hipMemcpyHostToDevice, e->ingS), "raw arena");
  // host buffers are reusable when lkf_ingest returns (the header's contract)
  HIPCHK(hipStreamSynchronize(e->ingS), "ingest copy sync");
  return ingest_common(e, x, x.dRawPkts, n, x.dArenaOwn, raw_len);
}

int lkf_ingest_device(lkf_engine *e, const lkf_raw_pkt *d_pkts, uint32_t n, const uint8_t *d_raw, uint64_t raw_len) {
  if (!e || (n && (!d_pkts || !d_raw))) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts) return LKF_ENOSPC;
  const auto t0 = std::chrono::steady_clock::now();
  int rc = flush_topology(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  BatchCtx &x = e->ctx[e->nRuns % lkf_engine::kCtx];
  if (x.used) HIPCHK(hipStreamWaitEvent(e->ingS, x.emitted, 0), "wait emit");
  rc = ingest_common(e, x, d_pkts, n, d_raw, raw_len);
  if (e->knobs.hostProf) {
    e->hp[7] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    e->hp[8] += 1;
  }
  return rc;
}

// ---- SRTP unprotect (in front of ingress) ---------------------------------------
static int srtp_rx_init(lkf_engine *e) {
  int rc = srtp_init(e);
  if (rc) return rc;
  if (e->dSrtpRx) return LKF_OK;
  const uint32_t mp = e->cfg.max_batch_pkts;
  HIPCHK(e->dSrtpRxSpec.alloc(e->maxStreams), "alloc srtp rx spec state");
  HIPCHK(e->dRxRange.alloc(2 * size_t(e->maxStreams)), "alloc srtp rx ranges");
  HIPCHK(e->dRxAuth.alloc(mp), "alloc srtp rx auth");
  HIPCHK(e->dRxSpec.alloc(mp), "alloc srtp rx spec");
  HIPCHK(e->dRxRes.alloc(mp), "alloc srtp rx results");
  for (auto &r : e->rxRing)
    for (auto &ev : r) HIPCHK(ev.create(true), "unprotect event");
  HIPCHK(e->dSrtpRx.alloc(e->maxStreams), "alloc srtp rx state");
  HIPCHK(hipMemsetAsync(e->dSrtpRx, 0, sizeof(SrtpRx) * e->maxStreams, e->own), "srtp rx init");
  HIPCHK(hipStreamSynchronize(e->own), "srtp rx init sync");
  return LKF_OK;
}

int lkf_set_stream_transport(lkf_engine *e, int32_t stream, int32_t t) {
  if (!e || stream < 0 || stream >= int32_t(e->streams.size()) || t < -1 || t >= int32_t(e->transports.size()))
    return LKF_EINVAL;
  int rc = srtp_rx_init(e);
  if (rc) return rc;
  rc = drain_streams(e);  // queued unprotect stages read the binding and the state
  if (rc) return rc;
  SrtpRx v;
  std::memset(&v, 0, sizeof(v));
  v.tp1 = uint32_t(t + 1);
  HIPCHK(hipMemcpy(e->dSrtpRx + stream, &v, sizeof(v), hipMemcpyHostToDevice), "srtp rx bind");
  return LKF_OK;
}

// Enqueues the unprotect stage on the ingest stream (no host sync).
static int unprotect_common(lkf_engine *e, const lkf_raw_pkt *dPkts, uint32_t n, const uint8_t *dSrtp,
                            uint64_t srtpLen, lkf_raw_pkt *dPktsOut, uint8_t *dPlain) {
  SrtpRxArgs a;
  a.tab = e->dAesTab;
  a.pkts = dPkts;
  a.n = n;
  a.nstreams = uint32_t(e->streams.size());
  a.srtp = dSrtp;
  a.srtpLen = srtpLen;
  a.pktsOut = dPktsOut;
  a.plain = dPlain;
  a.rx = e->dSrtpRx;
  a.rxSpec = e->dSrtpRxSpec;
  a.range = e->dRxRange;
  a.keys = e->dSrtpKeys;
  a.spec = e->dRxSpec;
  a.auth = e->dRxAuth;
  a.res = e->dRxRes;
  const size_t slot = e->nUnprotects % 256;
  HIPCHK(hipEventRecord(e->rxRing[slot][0], e->ingS), "event");
  HIPCHK(launch_srtp_unprotect(e->ingS, a), "unprotect");
  HIPCHK(hipEventRecord(e->rxRing[slot][1], e->ingS), "event");
  e->nUnprotects++;
  e->lastUnprotectN = n;
  return LKF_OK;
}

int lkf_unprotect_device(lkf_engine *e, const lkf_raw_pkt *d_pkts, uint32_t n, const uint8_t *d_srtp,
                         uint64_t srtp_len, lkf_raw_pkt *d_pkts_out, uint8_t *d_plain) {
  if (!e || (n && (!d_pkts || !d_srtp || !d_pkts_out || !d_plain))) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts) return LKF_ENOSPC;
  if (n) {
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(d_srtp), p0 = reinterpret_cast<uintptr_t>(d_plain);
    if ((s0 | p0) & 15) {
      e->err = "lkf_unprotect_device: the arenas must be 16-byte aligned";
      return LKF_EINVAL;
    }
    if (s0 < p0 + srtp_len && p0 < s0 + srtp_len) {
      e->err = "lkf_unprotect_device: the plaintext arena overlaps the input";
      return LKF_EINVAL;
    }
  }
  int rc = srtp_rx_init(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  return unprotect_common(e, d_pkts, n, d_srtp, srtp_len, d_pkts_out, d_plain);
}

int lkf_ingest_srtp(lkf_engine *e, const lkf_raw_pkt *pkts, uint32_t n, const uint8_t *srtp, uint64_t srtp_len) {
  if (!e || (n && (!pkts || !srtp))) return LKF_EINVAL;
  if (n > e->cfg.max_batch_pkts || srtp_len > e->cfg.max_batch_arena) return LKF_ENOSPC;
  int rc = flush_topology(e);
  if (rc) return rc;
  rc = srtp_rx_init(e);
  if (rc) return rc;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (!e->dSrtpStage) {
    HIPCHK(e->dSrtpStage.alloc(e->cfg.max_batch_arena + 64), "alloc srtp staging");
    HIPCHK(e->dSrtpPktsIn.alloc(e->cfg.max_batch_pkts), "alloc srtp staging");
  }
  BatchCtx &x = e->ctx[e->nRuns % lkf_engine::kCtx];
  rc = ingest_staging_waits(e, x);
  if (rc) return rc;
  if (n) HIPCHK(hipMemcpyAsync(e->dSrtpPktsIn, pkts, size_t(n) * sizeof(lkf_raw_pkt), hipMemcpyHostToDevice, e->ingS),
                "srtp pkts");
  if (srtp_len) HIPCHK(hipMemcpyAsync(e->dSrtpStage, srtp, srtp_len, hipMemcpyHostToDevice, e->ingS), "srtp arena");
  HIPCHK(hipStreamSynchronize(e->ingS), "ingest copy sync");  // the host buffers are reusable on return
  rc = unprotect_common(e, e->dSrtpPktsIn, n, e->dSrtpStage, srtp_len, x.dRawPkts, x.dArenaOwn);
  if (rc) return rc;
  return ingest_common(e, x, x.dRawPkts, n, x.dArenaOwn, srtp_len);
}

int lkf_unprotect_results(lkf_engine *e, lkf_srtp_rx_result *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = e->lastUnprotectN;
  if (cap < e->lastUnprotectN) return LKF_ENOSPC;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync");
  if (e->lastUnprotectN) D2H(out, e->dRxRes, size_t(e->lastUnprotectN) * sizeof(lkf_srtp_rx_result), "unprotect results");
  return LKF_OK;
}

int lkf_stream_srtp_get(lkf_engine *e, int32_t stream, lkf_stream_srtp *out) {
  if (!e || !out || stream < 0 || stream >= int32_t(e->streams.size())) return LKF_EINVAL;
  std::memset(out, 0, sizeof(*out));
  out->transport = -1;
  if (!e->dSrtpRx) return LKF_OK;  // no stream was ever bound
  STEP(quiesce(e, false));
  SrtpRx s;
  D2H(&s, e->dSrtpRx + stream, sizeof(s), "srtp rx state copy");
  out->s_l = s.sl;
  out->mask = s.mask;
  out->started = s.started;
  out->transport = int32_t(s.tp1) - 1;
  out->accepted = s.accepted;
  out->auth_failures = s.authFail;
  out->replays = s.replay;
  out->malformed = s.malformed;
  return LKF_OK;
}

int lkf_unprotect_timing_window(lkf_engine *e, uint32_t n, float *unprotect_ms) {
  if (!e || n == 0 || n > 256 || n > e->nUnprotects) return LKF_EINVAL;
  float sum = 0;
  for (uint64_t r = e->nUnprotects - n; r < e->nUnprotects; r++) {
    HIPCHK(hipEventSynchronize(e->rxRing[r % 256][1]), "evsync");
    float a = 0;
    HIPCHK(hipEventElapsedTime(&a, e->rxRing[r % 256][0], e->rxRing[r % 256][1]), "elapsed");
    sum += a;
  }
  if (unprotect_ms) *unprotect_ms = sum;
  return LKF_OK;
}

int lkf_ingest_flows(lkf_engine *e, lkf_flow *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = e->lastIngestN;
  if (cap < e->lastIngestN) return LKF_ENOSPC;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync");
  if (e->lastIngestN)
    D2H(out, e->ing[e->ingPar].flows, size_t(e->lastIngestN) * sizeof(lkf_flow), "flows");
  return LKF_OK;
}

int lkf_ingest_twcc(lkf_engine *e, uint32_t *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = e->lastIngestN;
  if (cap < e->lastIngestN) return LKF_ENOSPC;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync");
  if (e->lastIngestN)
    D2H(out, e->dTwcc, size_t(e->lastIngestN) * sizeof(uint32_t), "twcc");
  return LKF_OK;
}

int lkf_ingested(lkf_engine *e, lkf_pkt *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync");
  uint32_t n = 0;
  if (e->haveBatch) {
    n = e->curN;
    if (e->curNDev) {
      uint64_t t = 0;
      D2H(&t, e->curNDev, sizeof(t), "count copy");
      n = uint32_t(t);
    }
  }
  *n_out = n;
  if (cap < n) return LKF_ENOSPC;
  if (n && e->curOwned) D2H(out, e->curPkts, size_t(n) * sizeof(lkf_pkt), "ingested copy");
  if (n && !e->curOwned)  // the caller's device buffer (lkf_submit_device): not an engine allocation
    HIPCHK(hipMemcpy(out, e->curPkts, size_t(n) * sizeof(lkf_pkt), hipMemcpyDeviceToHost), "ingested copy");
  return LKF_OK;
}

int lkf_ingested_dd(lkf_engine *e, lkf_pkt_dd *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  uint32_t n = 0;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync");
  if (e->haveBatch) {
    n = e->curN;
    if (e->curNDev) {
      uint64_t t = 0;
      D2H(&t, e->curNDev, sizeof(t), "count copy");
      n = uint32_t(t);
    }
  }
  *n_out = n;
  if (cap < n) return LKF_ENOSPC;
  if (!n) return LKF_OK;
  if (e->curDD && e->curDDOwned)
    D2H(out, e->curDD, size_t(n) * sizeof(lkf_pkt_dd), "ingested dd copy");
  else if (e->curDD)  // the caller's device buffer (lkf_submit_dd_device)
    HIPCHK(hipMemcpy(out, e->curDD, size_t(n) * sizeof(lkf_pkt_dd), hipMemcpyDeviceToHost), "ingested dd copy");
  else
    std::memset(out, 0, size_t(n) * sizeof(lkf_pkt_dd));
  return LKF_OK;
}

int lkf_stream_stats_get(lkf_engine *e, int32_t sid, lkf_stream_stats *o) {
  if (!e || !o || sid < 0 || sid >= int32_t(e->streams.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  StreamHot h;
  D2H(&h, e->dStreamHot + sid, sizeof(h), "stream state copy");
  std::memset(o, 0, sizeof(*o));
  o->initialized = (h.flags & S_INIT) ? 1 : 0;
  o->ext_start_sn = h.snStart;  // WrapAround.GetExtendedStart = ET(start)
  o->ext_highest_sn = h.snExtHighest;
  o->ext_start_ts = h.tsStart;
  o->ext_highest_ts = h.tsExtHighest;
  o->packets_lost = h.packetsLost;
  o->packets_out_of_order = h.packetsOutOfOrder;
  o->packets_duplicate = h.packetsDuplicate;
  o->packets_padding = h.packetsPadding;
  o->bytes = h.bytes;
  o->header_bytes = h.headerBytes;
  o->bytes_duplicate = h.bytesDuplicate;
  o->bytes_padding = h.bytesPadding;
  o->frames = h.frames;
  o->nacks = h.nacks;
  if (e->dNack) {  // (the NACK queues keep the count: see NackState)
    uint64_t nq = 0;
    D2H(&nq, &e->dNack[sid].nacks, sizeof(nq), "stream nacks");
    o->nacks += nq;
  }
  o->first_time_ns = h.firstTime;
  o->highest_time_ns = h.highestTime;
  o->last_transit = h.lastTransit;
  o->last_jitter_ext_ts = h.lastJitterExtTs;
  o->jitter = h.jitter;
  o->max_jitter = h.maxJitter;
  D2H(o->gap_histogram, e->dRxGap + size_t(sid) * kGapWords, kGapBins * sizeof(uint32_t), "stream gap copy");
  return LKF_OK;
}

// The last ingest's NACK records and pairs compacted in datagram order into
// dNackOut / dNackPairsOut, on the side stream (behind the NACK queues of the
// ingest that produced them), which is idle on return; tot = {records, pairs}.
static int nack_compact_run(lkf_engine *e, uint64_t tot[2]) {
  tot[0] = tot[1] = 0;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (!e->dNack || !e->lastIngestN) return LKF_OK;
  const uint32_t n = e->lastIngestN;
  hipStream_t ps = e->sideS;
  const lkf_engine::IngSet &g = e->ing[e->ingPar];  // the last ingest's set
  HIPCHK(launch_nack_compact(ps, n, e->ingRaws, e->dStreams, g.nackInfo, g.nackPairOff, g.nackPairs,
                             e->dNackPartA, nullptr, e->dNackRecPos, e->dNackPairPos, e->dNackTot, e->dNackOut, e->dNackPairsOut),
         "nack compact");
  CHKRANGE(e->dNackTot, 2 * sizeof(uint64_t), "async d2h");
  HIPCHK(hipMemcpyAsync(tot, e->dNackTot, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, ps), "nack totals");
  HIPCHK(hipStreamSynchronize(ps), "nack sync");
  return LKF_OK;
}

int lkf_ingest_nacks(lkf_engine *e, lkf_rtcp_nack *out, uint32_t cap, lkf_nack_pair *pairs, uint32_t pair_cap,
                     uint32_t *n_out, uint32_t *n_pairs_out) {
  if (!e || !n_out || !n_pairs_out) return LKF_EINVAL;
  *n_out = *n_pairs_out = 0;
  uint64_t tot[2] = {0, 0};
  STEP(nack_compact_run(e, tot));
  *n_out = uint32_t(tot[0]);
  *n_pairs_out = uint32_t(tot[1]);
  if (tot[0] > cap || tot[1] > pair_cap) return LKF_ENOSPC;
  if (tot[0] && !out) return LKF_EINVAL;
  if (tot[1] && !pairs) return LKF_EINVAL;
  if (tot[0]) D2H(out, e->dNackOut, tot[0] * sizeof(lkf_rtcp_nack), "nack records");
  if (tot[1])
    D2H(pairs, e->dNackPairsOut, tot[1] * sizeof(lkf_nack_pair), "nack pairs");
  return LKF_OK;
}

// ---- ingress frame rate (ingress_kernels.hip k_ing_fps; the semantics are fps_device.h) ----
static_assert(LKF_FPS_NONE == fps::KIND_NONE && LKF_FPS_VP8 == fps::KIND_VP8 && LKF_FPS_VP9 == fps::KIND_VP9,
              "LKF_FPS_* are fps::KIND_*");
static_assert(sizeof(lkf_stream_fps) == 128 && sizeof(lkf_fps_calc) == 24, "lkf_stream_fps is 128 B");

static int fps_index(const lkf_engine *e, int32_t stream) {
  return size_t(stream) < e->fpsIdx.size() ? e->fpsIdx[stream] : -1;
}

static int fps_dd_index(const lkf_engine *e, int32_t stream) {
  return size_t(stream) < e->fpsDDIdx.size() ? e->fpsDDIdx[stream] : -1;
}

int lkf_stream_fps_enable(lkf_engine *e, int32_t stream) {
  if (!e || stream < 0 || stream >= int32_t(e->streams.size())) return LKF_EINVAL;
  const lkf_stream_params &sp = e->streams[stream];
  const lkf_track_params &tp = e->tracks[sp.track];
  // buffer.go:216-227: a calculator exists for video/vp8 and video/vp9; a
  // Buffer with a DD parser gets FrameRateCalculatorDD (buffer.go:193-198), which is not built
  if (tp.kind != LKF_KIND_VIDEO || (tp.codec != LKF_CODEC_VP8 && tp.codec != LKF_CODEC_VP9) || sp.dd_ext)
    return LKF_EINVAL;
  if (fps_index(e, stream) >= 0) return LKF_OK;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  const size_t n = e->fpsHandles.size();
  if (n + 1 > e->dFps.cap()) {  // grow: queued k_ing_fps launches hold the old pointers
    STEP(drain_streams(e));
    const size_t cap = std::max<size_t>(64, 2 * (n + 1));
    DevBuf<uint32_t> list, at;
    DevBuf<fps::State> st;
    HIPCHK(list.alloc(cap), "alloc fps list");
    HIPCHK(at.alloc(cap), "alloc fps epochs");
    HIPCHK(st.alloc(cap), "alloc fps state");
    if (n) {
      HIPCHK(hipMemcpy(list, e->dFpsList, n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "fps list copy");
      HIPCHK(hipMemcpy(at, e->dFpsCalcAt, n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "fps epochs copy");
      HIPCHK(hipMemcpy(st, e->dFps, n * sizeof(fps::State), hipMemcpyDeviceToDevice), "fps state copy");
    }
    e->dFpsList = std::move(list);
    e->dFpsCalcAt = std::move(at);
    e->dFps = std::move(st);
  }
  // (entry n is beyond every queued launch's grid: no wait)
  fps::State s;
  std::memset(&s, 0, sizeof(s));
  s.kind = tp.codec == LKF_CODEC_VP8 ? fps::KIND_VP8 : fps::KIND_VP9;
  s.clockRate = tp.clock_rate;
  s.stream = uint32_t(stream);
  const uint32_t h = uint32_t(stream), zero = 0;
  HIPCHK(hipMemcpy(e->dFps + n, &s, sizeof(s), hipMemcpyHostToDevice), "fps state init");
  HIPCHK(hipMemcpy(e->dFpsList + n, &h, sizeof(h), hipMemcpyHostToDevice), "fps list entry");
  HIPCHK(hipMemcpy(e->dFpsCalcAt + n, &zero, sizeof(zero), hipMemcpyHostToDevice), "fps epoch entry");
  if (e->fpsIdx.size() <= size_t(stream)) e->fpsIdx.resize(size_t(stream) + 1, -1);
  e->fpsIdx[stream] = int32_t(n);
  e->fpsHandles.push_back(stream);
  return LKF_OK;
}

int lkf_stream_fps_get(lkf_engine *e, int32_t stream, lkf_stream_fps *o) {
  if (!e || !o || stream < 0 || stream >= int32_t(e->streams.size())) return LKF_EINVAL;
  std::memset(o, 0, sizeof(*o));
  const int idx = fps_index(e, stream);
  if (idx < 0) {
    const int ddi = fps_dd_index(e, stream);
    if (ddi < 0) return LKF_OK;  // LKF_FPS_NONE
    STEP(quiesce(e));
    fpsdd::State d;
    D2H(&d, e->dFpsDD + ddi, sizeof(d), "fps dd state copy");
    o->kind = d.kind;
    o->calculated = uint8_t(d.calculated);
    // (all three frameRateCalculator[] entries are the one calculator, buffer.go:195-198)
    for (int c = 0; c < fpsdd::kSpatial; c++) {
      o->completed[c] = d.h.completed;
      for (int t = 0; t < fpsdd::kTemporal; t++) o->fps[c][t] = d.h.rate[c][t];
    }
    return LKF_OK;
  }
  STEP(quiesce(e));
  fps::State s;
  D2H(&s, e->dFps + idx, sizeof(s), "fps state copy");
  o->kind = s.kind;
  o->calculated = uint8_t(s.calculated);
  for (int c = 0; c < fps::kSpatial; c++) {
    const fps::Head &h = s.c[c].h;
    lkf_fps_calc &k = o->calc[c];
    o->completed[c] = h.completed;
    k.present = h.present;
    k.base_fn = h.baseFn;
    k.has_base = h.hasBase;
    k.resets = h.resets;
    for (int t = 0; t < fps::kTemporal; t++) {
      o->fps[c][t] = h.rate[t];
      k.first[t] = int8_t(int(fps::slot_of(h.first, t)) - 1);
      k.second[t] = int8_t(int(fps::slot_of(h.second, t)) - 1);
    }
  }
  return LKF_OK;
}

// ---- ... with a dependency descriptor (k_ing_fps_dd; the semantics are fps_dd_device.h) ----
static_assert(LKF_FPS_DD == fpsdd::KIND_DD, "LKF_FPS_DD is fpsdd::KIND_DD");
static_assert(sizeof(lkf_fps_dd) == 480, "lkf_fps_dd is 480 B");

int lkf_stream_fps_enable_dd(lkf_engine *e, int32_t stream) {
  if (!e || stream < 0 || stream >= int32_t(e->streams.size())) return LKF_EINVAL;
  const lkf_stream_params &sp = e->streams[stream];
  const lkf_track_params &tp = e->tracks[sp.track];
  // buffer.go:191-201: the calculator comes with the DD extension, whatever the video codec
  if (tp.kind != LKF_KIND_VIDEO || !sp.dd_ext) return LKF_EINVAL;
  if (fps_dd_index(e, stream) >= 0) return LKF_OK;
  STEP(quiesce(e));  // (the stream's parser state is read below; queued launches hold the old pointers)
  const size_t n = e->fpsDDHandles.size();
  if (n + 1 > e->dFpsDD.cap()) {
    const size_t cap = std::max<size_t>(16, 2 * (n + 1));
    DevBuf<uint32_t> list, at;
    DevBuf<fpsdd::State> st;
    DevBuf<DDStruct> ds;
    HIPCHK(list.alloc(cap), "alloc fps dd list");
    HIPCHK(at.alloc(cap), "alloc fps dd epochs");
    HIPCHK(st.alloc(cap), "alloc fps dd state");
    HIPCHK(ds.alloc(2 * cap), "alloc fps dd structures");
    HIPCHK(hipMemset(ds, 0, 2 * cap * sizeof(DDStruct)), "fps dd structures reset");
    if (n) {
      HIPCHK(hipMemcpy(list, e->dFpsDDList, n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "fps dd list copy");
      HIPCHK(hipMemcpy(at, e->dFpsDDCalcAt, n * sizeof(uint32_t), hipMemcpyDeviceToDevice), "fps dd epochs copy");
      HIPCHK(hipMemcpy(st, e->dFpsDD, n * sizeof(fpsdd::State), hipMemcpyDeviceToDevice), "fps dd state copy");
      HIPCHK(hipMemcpy(ds, e->dFpsDDStruct, 2 * n * sizeof(DDStruct), hipMemcpyDeviceToDevice),
             "fps dd structures copy");
    }
    e->dFpsDDList = std::move(list);
    e->dFpsDDCalcAt = std::move(at);
    e->dFpsDD = std::move(st);
    e->dFpsDDStruct = std::move(ds);
  }
  auto s = std::make_unique<fpsdd::State>();
  std::memset(s.get(), 0, sizeof(fpsdd::State));
  s->kind = fpsdd::KIND_DD;
  s->clockRate = tp.clock_rate;
  s->stream = uint32_t(stream);
  s->vp8 = tp.codec == LKF_CODEC_VP8;
  fpsdd::set_max_layer(s->h, 2, 3);  // DefaultMaxLayerSpatial / Temporal (fps.go:340-341)
  // A parser that already holds a structure: the calculator starts from it and
  // from the parser's active mask (no reference counterpart: DESIGN §2)
  uint32_t ddIdx = 0;
  for (int32_t k = 0; k < stream; k++) ddIdx += e->streams[k].dd_ext ? 1u : 0u;
  if (e->dDDIng && ddIdx < e->ddStreamInit) {
    auto ps = std::make_unique<DDIngState>();
    D2H(ps.get(), e->dDDIng + ddIdx, sizeof(DDIngState), "dd parser copy");
    if (ps->flags & DI_HAS_STRUCT) {
      const DDStruct *src = e->dDDIngStruct + size_t(ddIdx) * 2 + ((ps->flags & DI_CUR) ? 1 : 0);
      auto hs = std::make_unique<DDStruct>();
      D2H(hs.get(), src, sizeof(DDStruct), "dd parser structure copy");
      HIPCHK(hipMemcpy(e->dFpsDDStruct + 2 * n, src, sizeof(DDStruct), hipMemcpyDeviceToDevice),
             "fps dd structure seed");
      s->hasStruct = 1;
      const uint32_t ml = fpsdd::max_layer_of(ps->activeMask, hs->numDT, hs->dtTarget, hs->dtS, hs->dtT);
      fpsdd::set_max_layer(s->h, ml & 0xffu, ml >> 8);
    }
  }
  const uint32_t h = uint32_t(stream), zero = 0;
  HIPCHK(hipMemcpy(e->dFpsDD + n, s.get(), sizeof(fpsdd::State), hipMemcpyHostToDevice), "fps dd state init");
  HIPCHK(hipMemcpy(e->dFpsDDList + n, &h, sizeof(h), hipMemcpyHostToDevice), "fps dd list entry");
  HIPCHK(hipMemcpy(e->dFpsDDCalcAt + n, &zero, sizeof(zero), hipMemcpyHostToDevice), "fps dd epoch entry");
  if (e->fpsDDIdx.size() <= size_t(stream)) e->fpsDDIdx.resize(size_t(stream) + 1, -1);
  e->fpsDDIdx[stream] = int32_t(n);
  e->fpsDDHandles.push_back(stream);
  return LKF_OK;
}

int lkf_stream_fps_dd_get(lkf_engine *e, int32_t stream, lkf_fps_dd *o) {
  if (!e || !o || stream < 0 || stream >= int32_t(e->streams.size())) return LKF_EINVAL;
  const int idx = fps_dd_index(e, stream);
  if (idx < 0) return LKF_EINVAL;
  STEP(quiesce(e));
  auto s = std::make_unique<fpsdd::State>();
  D2H(s.get(), e->dFpsDD + idx, sizeof(fpsdd::State), "fps dd state copy");
  std::memset(o, 0, sizeof(*o));
  const fpsdd::Head &h = s->h;
  o->base_fn = h.baseFn;
  o->has_base = h.hasBase;
  o->completed = h.completed;
  o->max_spatial = h.maxSpatial;
  o->max_temporal = h.maxTemporal;
  o->resets = h.resets;
  fpsdd::HostWin w{s->ts, s->chain, s->layer};
  for (int j = 0; j < fpsdd::kWords; j++) o->present[j] = h.present[j];
  for (int c = 0; c < fpsdd::kSpatial; c++)
    for (int t = 0; t < fpsdd::kTemporal; t++) {
      const bool has = (h.has >> (4 * c + t)) & 1;
      o->first[c][t] = has ? int16_t(fpsdd::byte_of(h.first[c], t)) : int16_t(-1);
      o->second[c][t] = has ? int16_t(fpsdd::byte_of(h.second[c], t)) : int16_t(-1);
      for (int j = 0; j < fpsdd::kWords; j++) o->chain[c][t][j] = w.chain_word(4 * c + t, j);
    }
  return LKF_OK;
}

int lkf_ingest_fps_changed(lkf_engine *e, int32_t *streams, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  *n_out = 0;
  const size_t n = e->fpsHandles.size(), nd = e->fpsDDHandles.size();
  if ((!n && !nd) || !e->fpsEpoch) return LKF_OK;
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  HIPCHK(hipStreamSynchronize(e->ingS), "sync ingest stream");
  HIPCHK(hipStreamSynchronize(e->sideS), "sync side stream");  // (the calculators of the last ingest)
  std::vector<uint32_t> at(std::max(n, nd));
  std::vector<int32_t> hit;
  if (n) {
    D2H(at.data(), e->dFpsCalcAt, n * sizeof(uint32_t), "fps epochs copy");
    for (size_t i = 0; i < n; i++)
      if (at[i] == e->fpsEpoch) hit.push_back(e->fpsHandles[i]);
  }
  if (nd) {  // the dependency-descriptor calculators: merged (sorted below)
    D2H(at.data(), e->dFpsDDCalcAt, nd * sizeof(uint32_t), "fps dd epochs copy");
    for (size_t i = 0; i < nd; i++)
      if (at[i] == e->fpsEpoch) hit.push_back(e->fpsDDHandles[i]);
  }
  std::sort(hit.begin(), hit.end());
  *n_out = uint32_t(hit.size());
  if (hit.size() > cap) return LKF_ENOSPC;
  if (!hit.empty() && !streams) return LKF_EINVAL;
  if (!hit.empty()) std::memcpy(streams, hit.data(), hit.size() * sizeof(int32_t));
  return LKF_OK;
}

// The same list as rtcp.TransportLayerNack packets (k_nack_wire): record i at
// 12 * i + 4 * pair_off[i], so the arena is 12 * records + 4 * pairs bytes.
int lkf_ingest_nacks_wire(lkf_engine *e, lkf_stream_rtcp_pkt *pkts, uint32_t cap, uint8_t *arena, uint64_t arena_cap,
                          uint32_t *n_out, uint64_t *arena_len) {
  if (!e || !n_out || !arena_len) return LKF_EINVAL;
  *n_out = 0;
  *arena_len = 0;
  uint64_t tot[2] = {0, 0};
  STEP(nack_compact_run(e, tot));
  const uint64_t bytes = 12 * tot[0] + 4 * tot[1];
  if (bytes > 0xffffffffull) {
    e->err = "NACK packets of one ingest exceed 2^32 - 1 bytes";
    return LKF_EINVAL;
  }
  *n_out = uint32_t(tot[0]);
  *arena_len = bytes;
  if (tot[0] > cap || bytes > arena_cap) return LKF_ENOSPC;
  if (!tot[0]) return LKF_OK;
  if (!pkts || !arena) return LKF_EINVAL;
  // (the side stream is idle: the buffers grow without a wait)
  HIPCHK(e->dNackPkts.reserve(tot[0], 1024), "alloc nack packets");
  HIPCHK(e->dNackWire.reserve(bytes, 1 << 16), "alloc nack wire");
  NackWireLaunch a;
  a.recs = e->dNackOut;
  a.n = uint32_t(tot[0]);
  a.pairs = e->dNackPairsOut;
  a.npairs = tot[1];
  a.pkts = e->dNackPkts;
  a.arena = e->dNackWire;
  a.arenaCap = e->dNackWire.cap();
  HIPCHK(launch_nack_wire(e->sideS, a), "nack wire");
  HIPCHK(hipStreamSynchronize(e->sideS), "nack wire sync");
  D2H(pkts, e->dNackPkts, tot[0] * sizeof(lkf_stream_rtcp_pkt), "nack packets");
  D2H(arena, e->dNackWire, bytes, "nack wire bytes");
  return LKF_OK;
}

// ---- the publisher RTCP loop (rtcp_kernels.hip k_pub_*; the semantics are pub_rtcp_device.h) ----
static_assert(sizeof(lkf_stream_rtcp) == sizeof(StreamRtcp), "lkf_stream_rtcp is StreamRtcp's layout");
static_assert(offsetof(lkf_stream_rtcp, sr_newest) == offsetof(StreamRtcp, srNewest) &&
                  offsetof(lkf_stream_rtcp, snapshot_ext_start_sn) == offsetof(StreamRtcp, snapExtStartSN) &&
                  offsetof(lkf_stream_rtcp, start_time_ns) == offsetof(StreamRtcp, startTime) &&
                  offsetof(lkf_stream_rtcp, clock_skew_count) == offsetof(StreamRtcp, clockSkewCount),
              "lkf_stream_rtcp is StreamRtcp's layout");
static_assert(sizeof(lkf_stream_sr) == 16 && sizeof(lkf_stream_sr_result) == 24 && sizeof(lkf_stream_rr_req) == 8 &&
                  sizeof(lkf_stream_rr) == 40 && sizeof(lkf_stream_rtcp_raw) == 12 &&
                  sizeof(lkf_stream_rtcp_entry) == 8 && sizeof(lkf_stream_rtcp_in_result) == 32 &&
                  sizeof(lkf_stream_rtcp_pkt) == 16,
              "publisher RTCP call records");

int lkf_stream_rtcp_get(lkf_engine *e, int32_t sid, lkf_stream_rtcp *out) {
  if (!e || !out || sid < 0 || sid >= int32_t(e->streams.size())) return LKF_EINVAL;
  STEP(quiesce(e));
  D2H(out, e->dStreamRtcp + sid, sizeof(*out), "stream rtcp copy");
  return LKF_OK;
}

// The calls' frame is Order::Ingress: every queued stage waited for, the
// kernels on the ingest stream.  Their scratch is one family: input bytes,
// group bounds, result bytes; the compounds' arena is a family of its own.
static int pub_grow(Frame &f, size_t inBytes, size_t groups, size_t outBytes) {
  lkf_engine *e = f.e;
  return f.grow("alloc stream rtcp scratch", want(e->dPubIn, inBytes, 1 << 16, 2 * inBytes),
                want(e->dPubGroups, groups, 4096, 2 * groups), want(e->dPubOut, outBytes, 1 << 16, 2 * outBytes));
}

int lkf_stream_sender_reports(lkf_engine *e, const lkf_stream_sr *in, uint32_t n, int64_t now_ns,
                              lkf_stream_sr_result *out) {
  if (!e || (n && (!in || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  // groups: one per stream's contiguous entries (a stream must not reappear)
  std::vector<uint32_t> g;
  STEP(check_handles(&in[0].stream, sizeof(*in), n, e->streams.size(), {Repeat::Groups, &g, true}));
  Frame f(e, Order::Ingress);
  STEP(f.open());
  STEP(pub_grow(f, size_t(n) * sizeof(lkf_stream_sr), g.size(), size_t(n) * sizeof(lkf_stream_sr_result)));
  STEP(f.up(e->dPubIn, in, size_t(n) * sizeof(lkf_stream_sr), "stream sr copy"));
  STEP(f.up(e->dPubGroups, g.data(), g.size() * sizeof(uint32_t), "stream groups copy"));
  STEP(f.uploaded());
  PubSrLaunch a{};
  a.sr = reinterpret_cast<const lkf_stream_sr *>(e->dPubIn.get());
  a.n = n;
  a.gBegin = e->dPubGroups;
  a.ngroups = uint32_t(g.size() - 1);
  a.now = now_ns;
  a.streams = e->dStreams;
  a.hot = e->dStreamHot;
  a.rtcp = e->dStreamRtcp;
  a.nstreams = uint32_t(e->streams.size());
  a.srOut = reinterpret_cast<lkf_stream_sr_result *>(e->dPubOut.get());
  HIPCHK(launch_pub_sr_apply(f.s, a), "stream sr apply");
  STEP(f.down(out, e->dPubOut, size_t(n) * sizeof(lkf_stream_sr_result), "stream sr results copy"));
  return f.wait();
}

int lkf_stream_receiver_reports(lkf_engine *e, const lkf_stream_rr_req *req, uint32_t n, int64_t now_ns,
                                lkf_stream_rr *out, uint8_t *wire32) {
  if (!e || (n && (!req || !out))) return LKF_EINVAL;
  if (!n) return LKF_OK;
  // one thread per request: a stream's state has one writer
  STEP(check_handles(&req[0].stream, sizeof(*req), n, e->streams.size(), {Repeat::DistinctEorder}));
  // results: n records (40 B each, so the wire bytes behind them stay 4-B aligned), then 32 B per request
  const size_t recBytes = size_t(n) * sizeof(lkf_stream_rr), wireBytes = wire32 ? size_t(n) * 32 : 0;
  Frame f(e, Order::Ingress);
  STEP(f.open());
  STEP(pub_grow(f, size_t(n) * sizeof(lkf_stream_rr_req), 0, recBytes + wireBytes));
  STEP(f.up(e->dPubIn, req, size_t(n) * sizeof(lkf_stream_rr_req), "stream rr requests copy"));
  STEP(f.uploaded());
  PubRrLaunch a{};
  a.req = reinterpret_cast<const lkf_stream_rr_req *>(e->dPubIn.get());
  a.n = n;
  a.now = now_ns;
  a.streams = e->dStreams;
  a.hot = e->dStreamHot;
  a.rtcp = e->dStreamRtcp;
  a.nstreams = uint32_t(e->streams.size());
  a.out = reinterpret_cast<lkf_stream_rr *>(e->dPubOut.get());
  a.wire = wire32 ? e->dPubOut.get() + recBytes : nullptr;
  HIPCHK(launch_pub_rr_build(f.s, a), "stream rr build");
  STEP(f.down(out, e->dPubOut, recBytes, "stream rr results copy"));
  STEP(f.wait());
  if (wire32) D2H(wire32, e->dPubOut.get() + recBytes, wireBytes, "stream rr wire copy");
  return LKF_OK;
}

// `arena`: the compound packets in host memory, uploaded first; NULL: they are
// the arena_len bytes at dArena already (lkf_stream_rtcp_ingest_unprotected).
static int stream_rtcp_ingest_run(lkf_engine *e, const lkf_stream_rtcp_raw *in, uint32_t n, const uint8_t *arena,
                                  const uint8_t *dArena, uint64_t arena_len, int64_t now_ns,
                                  lkf_stream_rtcp_in_result *out) {
  if (!e || (n && (!in || !out)) || (arena_len && !arena && !dArena)) return LKF_EINVAL;
  if (!n) return LKF_OK;
  std::vector<uint32_t> g;
  STEP(check_handles(&in[0].stream, sizeof(*in), n, e->streams.size(), {Repeat::Groups, &g, true}, [&](uint32_t i) {
    return in[i].len <= LKF_RTCP_MAX_LEN && uint64_t(in[i].off) + in[i].len <= arena_len;
  }));
  Frame f(e, Order::Ingress);
  STEP(f.open());
  STEP(pub_grow(f, size_t(n) * sizeof(lkf_stream_rtcp_raw), g.size(), size_t(n) * sizeof(lkf_stream_rtcp_in_result)));
  if (arena) STEP(f.grow("alloc stream rtcp arena", want(e->dPubArena, arena_len, 1 << 16, 2 * arena_len)));
  STEP(f.up(e->dPubIn, in, size_t(n) * sizeof(lkf_stream_rtcp_raw), "stream rtcp raw copy"));
  if (arena && arena_len) STEP(f.up(e->dPubArena, arena, arena_len, "stream rtcp arena copy"));
  STEP(f.up(e->dPubGroups, g.data(), g.size() * sizeof(uint32_t), "stream groups copy"));
  STEP(f.uploaded());
  PubSrLaunch a{};
  a.raw = reinterpret_cast<const lkf_stream_rtcp_raw *>(e->dPubIn.get());
  a.n = n;
  a.arena = arena ? e->dPubArena.get() : dArena;
  a.arenaLen = arena_len;
  a.gBegin = e->dPubGroups;
  a.ngroups = uint32_t(g.size() - 1);
  a.now = now_ns;
  a.streams = e->dStreams;
  a.hot = e->dStreamHot;
  a.rtcp = e->dStreamRtcp;
  a.nstreams = uint32_t(e->streams.size());
  a.res = reinterpret_cast<lkf_stream_rtcp_in_result *>(e->dPubOut.get());
  HIPCHK(launch_pub_rtcp_check(f.s, a), "stream rtcp check");
  HIPCHK(launch_pub_sr_apply(f.s, a), "stream sr apply");
  STEP(f.down(out, e->dPubOut, size_t(n) * sizeof(lkf_stream_rtcp_in_result), "stream rtcp results copy"));
  return f.wait();
}

int lkf_stream_rtcp_ingest(lkf_engine *e, const lkf_stream_rtcp_raw *in, uint32_t n, const uint8_t *arena,
                           uint64_t arena_len, int64_t now_ns, lkf_stream_rtcp_in_result *out) {
  if (arena_len && !arena) return LKF_EINVAL;
  static const uint8_t none = 0;  // (an empty arena is still the caller's)
  return stream_rtcp_ingest_run(e, in, n, arena ? arena : &none, nullptr, arena_len, now_ns, out);
}

int lkf_stream_rtcp_ingest_unprotected(lkf_engine *e, const lkf_stream_rtcp_entry *in, uint32_t n, int64_t now_ns,
                                       lkf_stream_rtcp_in_result *out) {
  if (!e || (n && !in)) return LKF_EINVAL;
  std::vector<lkf_stream_rtcp_raw> raw(n);
  for (uint32_t i = 0; i < n; i++) {
    if (in[i].dgram >= e->scOff.size()) return LKF_EINVAL;
    const uint32_t len = e->scLen[in[i].dgram];  // (a rejected datagram: an empty entry at the arena's start)
    raw[i] = lkf_stream_rtcp_raw{in[i].stream, len ? e->scOff[in[i].dgram] : 0u, len};
  }
  static const uint8_t none = 0;  // (no datagram was accepted yet: every entry has len 0)
  const uint8_t *host = e->dScPlain ? nullptr : &none;
  return stream_rtcp_ingest_run(e, raw.data(), n, host, e->dScPlain, host ? 0 : e->scPlainLen, now_ns, out);
}

int lkf_stream_set_rtt(lkf_engine *e, int32_t sid, uint32_t rtt_ms) {
  if (!e || sid < 0 || sid >= int32_t(e->streams.size())) return LKF_EINVAL;
  if (rtt_ms == 0) return LKF_OK;  // Buffer.SetRTT ignores 0
  int rc = flush_topology(e);
  if (rc) return rc;
  // (not quiesce(): a stream without a NackQueue returns between the flush and the drain)
  if (!e->streams[sid].nack || !e->dNack) return LKF_OK;  // no NackQueue (the rtpStats RTT is out of scope)
  rc = drain_streams(e);  // a queued ingest reads the RTT
  if (rc) return rc;
  e->streams[sid].rtt_ms = rtt_ms;
  return write_row(e, &e->dNack[sid].rtt, rtt_ms, "nack rtt");
}

// Room -> participant -> microphone-stream tables for k_speakers.
static int rebuild_speakers(lkf_engine *e) {
  // primary receiver of a track = its layer-0 stream (first added)
  std::vector<int> primary(e->tracks.size(), -1);
  for (size_t sid = 0; sid < e->streams.size(); sid++) {
    const auto &sp = e->streams[sid];
    if (sp.layer == 0 && primary[sp.track] < 0) primary[sp.track] = int(sid);
  }
  // (room, participant) -> mic streams with an AudioLevel
  std::vector<std::pair<std::pair<uint32_t, uint32_t>, uint32_t>> rows;
  for (size_t t = 0; t < e->tracks.size(); t++) {
    const auto &tp = e->tracks[t];
    if (!tp.is_mic || !e->trackActive[t] || primary[t] < 0 || !e->streams[primary[t]].audio_level_ext) continue;
    rows.push_back({{tp.room, tp.publisher}, uint32_t(primary[t])});
  }
  std::stable_sort(rows.begin(), rows.end(),
                   [](const auto &a, const auto &b) { return a.first < b.first; });
  std::vector<uint32_t> roomOff, roomId, partId, partMicOff, mics;
  for (size_t i = 0; i < rows.size();) {
    const uint32_t room = rows[i].first.first;
    roomId.push_back(room);
    roomOff.push_back(uint32_t(partId.size()));
    while (i < rows.size() && rows[i].first.first == room) {
      const uint32_t part = rows[i].first.second;
      partId.push_back(part);
      partMicOff.push_back(uint32_t(mics.size()));
      while (i < rows.size() && rows[i].first.first == room && rows[i].first.second == part) mics.push_back(rows[i++].second);
    }
    if (partId.size() - roomOff.back() > 64) {
      e->err = "more than 64 microphone participants in a room";
      return LKF_ENOSPC;
    }
  }
  roomOff.push_back(uint32_t(partId.size()));
  partMicOff.push_back(uint32_t(mics.size()));
  e->nRooms = uint32_t(roomId.size());
  e->spkRoomIds = roomId;
  e->topoGen++;
  DevBuf<uint32_t> *bufs[] = {&e->dRoomPartOff, &e->dPartId, &e->dPartMicOff, &e->dMics, &e->dRoomId};
  const std::vector<uint32_t> *src[] = {&roomOff, &partId, &partMicOff, &mics, &roomId};
  for (int i = 0; i < 5; i++) {
    HIPCHK(bufs[i]->alloc(std::max<size_t>(src[i]->size(), 1)), "alloc speakers table");
    if (!src[i]->empty())
      HIPCHK(hipMemcpy(*bufs[i], src[i]->data(), src[i]->size() * sizeof(uint32_t), hipMemcpyHostToDevice),
             "speakers table copy");
  }
  const size_t slots = size_t(e->nRooms) * 64;
  if (e->dSpkSlots.cap() < slots || (slots && e->dSpkCounts.cap() < slots / 64 + 1)) {
    release_all(e->dSpkSlots, e->dSpkCounts);
    HIPCHK(e->dSpkSlots.alloc(std::max<size_t>(slots, 64)), "alloc slots");
    HIPCHK(e->dSpkCounts.alloc(std::max<size_t>(slots, 64) / 64 + 1), "alloc counts");
  }
  e->spkDirty = false;
  return LKF_OK;
}

// The speaker tick without a host wait: the ranking of every room at now_ns
// is enqueued on the prep stream (after the ingest that updated the levels)
// and stays in HBM (the per-room slots an all-gather reads); lkf_speakers
// reads a ranking back.
int lkf_speakers_enqueue(lkf_engine *e, int64_t now_ns) {
  if (!e) return LKF_EINVAL;
  int rc = flush_topology(e);
  if (rc) return rc;
  if (e->spkDirty) {
    rc = drain_streams(e);
    if (rc) return rc;
    rc = rebuild_speakers(e);
    if (rc) return rc;
  }
  if (e->nRooms == 0) return LKF_OK;
  SpeakersLaunch a;
  a.nrooms = e->nRooms;
  a.roomPartOff = e->dRoomPartOff;
  a.partId = e->dPartId;
  a.partMicOff = e->dPartMicOff;
  a.mics = e->dMics;
  a.roomId = e->dRoomId;
  a.streams = e->dStreams;
  a.hot = e->dStreamHot;
  a.nowNs = now_ns;
  a.slots = e->dSpkSlots;
  a.counts = e->dSpkCounts;
  HIPCHK(launch_speakers(e->ingS, a), "speakers");
  return LKF_OK;
}

int lkf_speakers(lkf_engine *e, int64_t now_ns, lkf_speaker *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  STEP(quiesce(e));
  if (e->spkDirty) STEP(rebuild_speakers(e));
  *n_out = 0;
  if (e->nRooms == 0) return LKF_OK;
  SpeakersLaunch a;
  a.nrooms = e->nRooms;
  a.roomPartOff = e->dRoomPartOff;
  a.partId = e->dPartId;
  a.partMicOff = e->dPartMicOff;
  a.mics = e->dMics;
  a.roomId = e->dRoomId;
  a.streams = e->dStreams;
  a.hot = e->dStreamHot;
  a.nowNs = now_ns;
  a.slots = e->dSpkSlots;
  a.counts = e->dSpkCounts;
  // the ingest stream: ordered after the ingest that updated the levels
  HIPCHK(launch_speakers(e->ingS, a), "speakers");
  std::vector<uint32_t> counts(e->nRooms);
  std::vector<lkf_speaker> slots(size_t(e->nRooms) * 64);
  CHKRANGE(e->dSpkCounts, counts.size() * sizeof(uint32_t), "async d2h");
  HIPCHK(hipMemcpyAsync(counts.data(), e->dSpkCounts, counts.size() * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        e->ingS),
         "counts copy");
  CHKRANGE(e->dSpkSlots, slots.size() * sizeof(lkf_speaker), "async d2h");
  HIPCHK(hipMemcpyAsync(slots.data(), e->dSpkSlots, slots.size() * sizeof(lkf_speaker), hipMemcpyDeviceToHost,
                        e->ingS),
         "slots copy");
  HIPCHK(hipStreamSynchronize(e->ingS), "speakers sync");
  uint32_t k = 0;
  for (uint32_t r = 0; r < e->nRooms; r++) k += counts[r];
  *n_out = k;
  if (cap < k) return LKF_ENOSPC;
  k = 0;
  for (uint32_t r = 0; r < e->nRooms; r++)
    for (uint32_t j = 0; j < counts[r]; j++) out[k++] = slots[size_t(r) * 64 + j];
  return LKF_OK;
}

// The room manager's periodic summary without a host wait (see lkfwd.h).
// The ranking and its pack run on the ingest stream after the last enqueued
// ingest; the totals' pack on the decide stream after the last enqueued
// decide (the DownTracks' sendingPacket totals); the caller's stream waits
// for both.  The engine never waits for the caller: the caller keeps `spk` /
// `bwe` unread by earlier work of its own until this tick's writes land
// (bench.py: a ring of buffers, each reused after its gather's event).
int lkf_room_summaries_enqueue(lkf_engine *e, int64_t now_ns, const uint32_t *room_ids, uint32_t rows, int32_t *spk,
                               uint32_t k, int64_t *bwe, uint32_t s, void *stream) {
  if (!e || (rows && !room_ids) || !spk || !bwe || k == 0 || k > 64 || s == 0) return LKF_EINVAL;
  for (uint32_t r = 1; r < rows; r++)
    if (room_ids[r] <= room_ids[r - 1]) return LKF_EINVAL;  // ascending, distinct
  int rc = flush_topology(e);
  if (rc) return rc;
  if (e->spkDirty) {
    rc = drain_streams(e);
    if (rc) return rc;
    rc = rebuild_speakers(e);
    if (rc) return rc;
  }
  HIPCHK(hipSetDevice(e->dev), "hipSetDevice");
  if (!e->rsSpk) {
    HIPCHK(e->rsSpk.create(false), "event");
    HIPCHK(e->rsDec.create(false), "event");
  }
  const uint32_t nd = uint32_t(e->dtp.size());
  if (rows != e->rsRooms.size() || !std::equal(room_ids, room_ids + rows, e->rsRooms.begin()) || k != e->rsK ||
      s != e->rsS || e->topoGen != e->rsGen) {
    std::vector<uint32_t> rooms(room_ids, room_ids + rows);
    auto rowOf = [&](uint32_t room) -> int32_t {
      auto it = std::lower_bound(rooms.begin(), rooms.end(), room);
      return it != rooms.end() && *it == room ? int32_t(it - rooms.begin()) : -1;
    };
    std::vector<int32_t> rowEng(std::max<uint32_t>(rows, 1), -1);
    for (uint32_t r = 0; r < e->nRooms; r++) {
      const int32_t row = rowOf(e->spkRoomIds[r]);
      if (row < 0) {
        e->err = "room_summaries: a room with microphones is not among room_ids";
        return LKF_EINVAL;
      }
      rowEng[row] = int32_t(r);
    }
    // active DownTracks by (row, subscriber, handle); a room's first s subscribers get slots
    std::vector<std::tuple<int32_t, uint32_t, uint32_t>> by;
    for (uint32_t d = 0; d < nd; d++) {
      if (!e->active[d]) continue;
      const int32_t row = rowOf(e->tracks[e->dtp[d].track].room);
      if (row < 0) {
        e->err = "room_summaries: a DownTrack's room is not among room_ids";
        return LKF_EINVAL;
      }
      by.emplace_back(row, e->dtp[d].subscriber, d);
    }
    std::sort(by.begin(), by.end());
    const size_t nslots = size_t(std::max<uint32_t>(rows, 1)) * s;
    std::vector<uint32_t> off(nslots + 1, 0), dts;
    std::vector<int64_t> sub(nslots, -1);
    std::vector<uint32_t> cnt(nslots, 0);
    for (size_t i = 0; i < by.size();) {
      const int32_t row = std::get<0>(by[i]);
      uint32_t pos = 0;
      while (i < by.size() && std::get<0>(by[i]) == row) {
        const uint32_t su = std::get<1>(by[i]);
        size_t j = i;
        while (j < by.size() && std::get<0>(by[j]) == row && std::get<1>(by[j]) == su) j++;
        if (pos < s) {
          const size_t slot = size_t(row) * s + pos;
          sub[slot] = su;
          cnt[slot] = uint32_t(j - i);
        }
        pos++;
        i = j;
      }
    }
    for (size_t q = 0; q < nslots; q++) off[q + 1] = off[q] + cnt[q];
    dts.resize(std::max<uint32_t>(off[nslots], 1));
    {
      std::vector<uint32_t> fillp(off.begin(), off.end() - 1);
      size_t i = 0;
      while (i < by.size()) {
        const int32_t row = std::get<0>(by[i]);
        uint32_t pos = 0;
        while (i < by.size() && std::get<0>(by[i]) == row) {
          const uint32_t su = std::get<1>(by[i]);
          while (i < by.size() && std::get<0>(by[i]) == row && std::get<1>(by[i]) == su) {
            if (pos < s) dts[fillp[size_t(row) * s + pos]++] = std::get<2>(by[i]);
            i++;
          }
          pos++;
        }
      }
    }
    HIPCHK(hipStreamSynchronize(e->ingS), "sync ingest stream");  // (a queued pack may read the old layout)
    HIPCHK(hipStreamSynchronize(e->decS), "sync decide stream");
    release_all(e->dRsRowEng, e->dRsSlotOff, e->dRsSlotDts, e->dRsSlotSub);
    HIPCHK(e->dRsRowEng.alloc(rowEng.size()), "alloc");
    HIPCHK(e->dRsSlotOff.alloc(off.size()), "alloc");
    HIPCHK(e->dRsSlotDts.alloc(dts.size()), "alloc");
    HIPCHK(e->dRsSlotSub.alloc(sub.size()), "alloc");
    HIPCHK(hipMemcpy(e->dRsRowEng, rowEng.data(), rowEng.size() * 4, hipMemcpyHostToDevice), "copy");
    HIPCHK(hipMemcpy(e->dRsSlotOff, off.data(), off.size() * 4, hipMemcpyHostToDevice), "copy");
    HIPCHK(hipMemcpy(e->dRsSlotDts, dts.data(), dts.size() * 4, hipMemcpyHostToDevice), "copy");
    HIPCHK(hipMemcpy(e->dRsSlotSub, sub.data(), sub.size() * 8, hipMemcpyHostToDevice), "copy");
    e->rsRooms = rooms;
    e->rsK = k;
    e->rsS = s;
    e->rsGen = e->topoGen;
  }
  hipStream_t cs = reinterpret_cast<hipStream_t>(stream);
  if (e->nRooms) {
    SpeakersLaunch a;
    a.nrooms = e->nRooms;
    a.roomPartOff = e->dRoomPartOff;
    a.partId = e->dPartId;
    a.partMicOff = e->dPartMicOff;
    a.mics = e->dMics;
    a.roomId = e->dRoomId;
    a.streams = e->dStreams;
    a.hot = e->dStreamHot;
    a.nowNs = now_ns;
    a.slots = e->dSpkSlots;
    a.counts = e->dSpkCounts;
    HIPCHK(launch_speakers(e->ingS, a), "speakers");
  }
  RoomPackLaunch p;
  p.rows = rows;
  p.k = k;
  p.s = s;
  p.rowEng = e->dRsRowEng;
  p.slots = e->dSpkSlots;
  p.counts = e->dSpkCounts;
  p.slotOff = e->dRsSlotOff;
  p.slotDts = e->dRsSlotDts;
  p.slotSub = e->dRsSlotSub;
  p.cum = e->dDTCum;
  p.spk = spk;
  p.bwe = bwe;
  // the ranking's pack right behind the ranking (ingest stream), the totals'
  // right behind the last enqueued decide: each reads its source before the
  // next ingest / decide on its stream can change it, and nothing of the
  // engine waits for the caller
  HIPCHK(launch_room_pack(e->ingS, e->decS, p), "room pack");
  HIPCHK(hipEventRecord(e->rsSpk, e->ingS), "event");
  HIPCHK(hipEventRecord(e->rsDec, e->decS), "event");
  HIPCHK(hipStreamWaitEvent(cs, e->rsSpk, 0), "wait");
  HIPCHK(hipStreamWaitEvent(cs, e->rsDec, 0), "wait");
  return LKF_OK;
}

// Not part of include/lkfwd.h: the bounds-check record of a checked build
// (-DLKF_CHECKED=1, liblkfwd_checked.so): {violations, first site, index,
// capacity}; LKF_ENODEV from a product build.
// Not part of include/lkfwd.h: the SVC-run stop counters of a diagnostic
// build (-DLKF_SVC_STATS=1; forward_kernels.hip g_svc), after a drain.
int lkf_debug_svc_stats(lkf_engine *e, uint64_t out[64], int reset) {
  if (!e || !out) return LKF_EINVAL;
  int rc = drain_streams(e);
  if (rc) return rc;
  unsigned long long v[64];
  const hipError_t r = read_svc_stats(v, reset);
  for (int i = 0; i < 64; i++) out[i] = v[i];
  return r == hipSuccess ? LKF_OK : LKF_ENODEV;
}

int lkf_debug_check(lkf_engine *e, uint64_t out[4], int reset) {
  if (!out) return LKF_EINVAL;
  if (e) {
    int rc = drain_streams(e);
    if (rc) return rc;
  } else if (hipDeviceSynchronize() != hipSuccess) {  // no engine: the whole device
    return LKF_EHIP;
  }
  unsigned long long v[4];
  hipError_t r = read_check(v, reset);
  for (int i = 0; i < 4; i++) out[i] = v[i];
  {  // the RTCP kernels keep their own record (rtcp_kernels.hip is its own code object)
    unsigned long long w[4];
    if (read_check_rtcp(w, reset) == hipSuccess && w[0]) {
      if (!out[0]) out[1] = w[1], out[2] = w[2], out[3] = w[3];
      out[0] += w[0];
    }
  }
  // host-side device -> host range violations (CHKRANGE) count as well, in
  // every build; site 0xD2H marks one when the device recorded none
  // an engine's own refusals; with no engine, every engine's
  std::atomic<uint64_t> &ctr = e ? e->rangeViolations : gRangeViolationsAll;
  const uint64_t rv = reset ? ctr.exchange(0) : ctr.load();
  if (rv) {
    if (!out[0]) out[1] = 0xD2, out[2] = 0, out[3] = 0;
    out[0] += rv;
    return LKF_OK;
  }
  return r == hipSuccess ? LKF_OK : LKF_ENODEV;
}

// Not part of include/lkfwd.h: every batch context's DD arena and spill bump
// cursors (out[2c], out[2c+1]) after a drain, and the arena's capacity
// (out[6]); LKF_EINVAL before the DD tables exist.  tests/test_dd_recapture_gpu.py
// checks them after graph re-captures forced under queued runs.
int lkf_debug_dd_cursors(lkf_engine *e, uint64_t out[7]) {
  if (!e || !out || !e->ddAlloc) return LKF_EINVAL;
  STEP(quiesce(e, false));
  for (int c = 0; c < lkf_engine::kCtx; c++) {
    uint64_t u[2] = {0, 0};
    D2H(u, e->ctx[c].dDDUsed, sizeof(u), "dd cursor copy");
    out[2 * c] = u[0];
    out[2 * c + 1] = u[1] & 0xffffffffu;
  }
  out[6] = e->ctx[0].dDDArena.cap();
  return LKF_OK;
}

// Not part of include/lkfwd.h: a DD DownTrack's selector state for debugging
// (out[16]: cache init, base, last, masks[8], chain broken bits, chain active
// bits, frames the unbroken chains wait on, frame-number wrapper last, current layers
// spatial | temporal << 8 (+128 each)).
int lkf_debug_dd_state(lkf_engine *e, int32_t dt, uint64_t out[16]) {
  if (!e || !out || dt < 0 || size_t(dt) >= e->dtp.size() || !e->dDDState) return LKF_EINVAL;
  STEP(quiesce(e, false));
  DDState d;
  DTHot h;
  D2H(&d, e->dDDState + dt, sizeof(d), "dd state");
  D2H(&h, e->dHot + dt, sizeof(h), "hot state");
  out[0] = (d.flags & DS_CACHE_INIT) ? 1 : 0;
  out[1] = d.cBase;
  out[2] = d.cLast;
  for (int i = 0; i < 8; i++) out[3 + i] = d.masks[i];
  const uint32_t cm = d.numChains >= 32 ? ~0u : (1u << d.numChains) - 1;
  out[11] = d.chBroken & cm;
  out[12] = d.chActive & cm;
  uint64_t ex = 0;
  for (int c = 0; c < d.numChains; c++) {  // (the set's size: the ring's bits and the frame beyond it)
    if ((d.chBroken >> c) & 1) continue;    // (a broken chain's set is inert until it is cleared)
    ex += d.expFar[c] ? 1 : 0;
    for (int w = 0; w < kDDExpWords; w++) ex += uint64_t(__builtin_popcountll(d.exp[c][w]));
  }
  out[13] = ex;
  out[14] = (d.flags & DS_FN_INIT) ? d.fnLast : ~0ull;
  out[15] = uint64_t(uint8_t(h.curS + 128)) | (uint64_t(uint8_t(h.curT + 128)) << 8);
  return LKF_OK;
}

int lkf_downtrack_summaries(lkf_engine *e, lkf_dt_summary *out, uint32_t cap, uint32_t *n_out) {
  if (!e || !n_out) return LKF_EINVAL;
  const uint32_t nd = uint32_t(e->dtp.size());
  *n_out = nd;
  if (cap < nd) return LKF_ENOSPC;
  if (!nd) return LKF_OK;
  if (!out) return LKF_EINVAL;
  STEP(quiesce(e));
  std::vector<DTCum> c(nd);
  D2H(c.data(), e->dDTCum, nd * sizeof(DTCum), "dt totals copy");
  for (uint32_t d = 0; d < nd; d++) {
    lkf_dt_summary &s = out[d];
    s.dt = int32_t(d);
    s.subscriber = e->dtp[d].subscriber;
    s.room = e->tracks[e->dtp[d].track].room;
    s.flags = (e->active[d] ? LKF_DTS_ACTIVE : 0u) | ((c[d].flags & F_DEFICIENT) ? LKF_DTS_DEFICIENT : 0u);
    s.packets_sent = c[d].packets;
    s.bytes_sent = c[d].bytes;
  }
  return LKF_OK;
}

int lkf_get_cumulative(lkf_engine *e, lkf_stats *out, int reset) {
  if (!e || !out) return LKF_EINVAL;
  int rc = drain_streams(e);
  if (rc) return rc;
  uint64_t st[kStatsWords];
  D2H(st, e->dCum, sizeof(st), "cum copy");
  out->tuples = st[0];
  out->forwarded = st[1];
  out->out_bytes = st[2];
  out->arena_bytes = st[3];
  for (int i = 0; i < LKF_DROP_NREASONS; i++) out->drops[i] = st[4 + i];
  if (reset) {
    HIPCHK(hipMemset(e->dCum, 0, sizeof(st)), "cum reset");
    HIPCHK(hipDeviceSynchronize(), "cum reset sync");  // before the next run's k_accumulate (emit stream)
  }
  return LKF_OK;
}

}  // extern "C"
