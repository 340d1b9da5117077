// reassembler.cpp -- e2sar::Reassembler over the gfx950 reassembly kernel.
//
// Reference: N receive threads, each owning a set of UDP ports, run the per-datagram body
// (e2sarDPReassembler.cpp:293-433) -- malloc, recvfrom, header checks, map lookup, memcpy
// -- one datagram at a time; a GC thread drops stale events (cpp:236-291).
// Here the receive threads only fill pinned datagram batches with recvmmsg (a slot of
// recvStride bytes per datagram); one device thread pipelines the batches through HBM:
// the host->device copy of batch b+1 runs on a copy stream beside the reassembly kernel of
// batch b (two device datagram buffers), a host batch goes back to the receive threads as
// soon as its copy has landed, and the events batch b completed leave the device arena in
// ONE gather launch into pinned staging, from which they are copied into the new[] buffers
// that getEvent/recvEvent hand over.  Lost-event records are drained the same way; the
// device GC pass runs every eventTimeout_ms; the table and arena are recycled or compacted
// when either passes half full.
#include <poll.h>
#include <sys/socket.h>

#include <algorithm>
#include <cerrno>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <thread>

#include "host_common.hpp"

namespace e2sar {

struct Reassembler::Impl {
    EjfatURI uri;
    ReassemblerFlags flags;
    std::string dataIP;
    bool v6 = false;
    uint16_t dataPort;
    int portRange;
    size_t numRecvThreads;
    size_t numRecvPorts;
    std::vector<std::vector<uint16_t>> threadsToPorts;

    // device: the compute stream (the context's) and a copy stream; two device datagram
    // buffers so batch b+1 is copied in while batch b is reassembled.
    // Teardown is the reverse of this declaration order, from `batches` up to `copyStream`:
    // ~Impl first synchronises both streams; then the pinned batches and staging, the
    // reassembler, the device sets and the events go, all before the context; the context is
    // destroyed while its stream is alive (e2sar_hip_ctx_destroy synchronises it); the
    // streams go last.
    detail::Stream copyStream;
    detail::Stream stream;
    detail::Ctx ctx;
    detail::Event gatherDone;           // recorded on the compute stream after a drain's gather
    struct DevSet {
        detail::DeviceBuf<uint8_t> pkts;
        detail::DeviceBuf<uint32_t> lens;
        detail::Event h2dDone;          // recorded on the copy stream after the batch's copy
    };
    DevSet sets[2];
    detail::Reas reas;
    detail::Pinned<uint8_t> stage;      // pinned staging for completed events
    size_t stageBytes = 0;
    struct Batch {                      // a datagram batch (pinned)
        detail::Pinned<uint8_t> pkts;
        detail::Pinned<uint32_t> lens;
        uint32_t n = 0;
    };
    std::vector<Batch> batches;

    std::vector<size_t> stageOffs;      // staging offsets of the records of the gather in flight
    std::atomic<uint64_t> upkeeps{0};   // recycles + compactions done
    std::vector<e2sar_hip_event_rec> recs;
    std::vector<e2sar_hip_lost_rec> lrecs;

    // queues of datagram batches between the receive threads and the device thread
    std::mutex bMu;
    std::condition_variable bFreeCv, bFullCv;
    std::deque<Batch *> freeB, fullB;

    // event queue (hpp:126-127: unbounded, see gatherFinish) and lost events (hpp:102-122, 262-279)
    struct Ev {
        std::unique_ptr<uint8_t[]> event;      // released to the caller of getEvent/recvEvent
        size_t bytes;
        EventNum_t eventNum;
        uint16_t dataId;
    };
    std::mutex eMu;
    std::condition_variable eCv;
    std::deque<Ev> evq;
    std::mutex lMu;
    std::deque<std::tuple<EventNum_t, uint16_t, size_t>> lostq;
    std::set<std::pair<EventNum_t, uint16_t>> lostSeen;

    // host-side counters
    std::atomic<uint64_t> hostEnqueueLoss{0};
    std::atomic<int> lastErrno{0}, dataErrCnt{0};
    std::atomic<E2SARErrorc> lastErr{E2SARErrorc::NoError};
    std::map<uint16_t, std::atomic<size_t> *> perPort;
    std::vector<std::unique_ptr<std::atomic<size_t>>> perPortStore;

    std::vector<std::thread> recvThreads;
    std::thread devThread;
    std::atomic<bool> stop{false};
    std::atomic<int> recvActive{0};
    bool started = false;
    e2sar_hip_reas_stats lastStats{};
    std::mutex sMu;

    Impl(const EjfatURI &u, const ReassemblerFlags &f, const std::string &ip, uint16_t port)
        : uri(u), flags(f), dataIP(ip), v6(ip.find(':') != std::string::npos), dataPort(port)
    {
    }
    ~Impl();
    void setup(size_t nThreads);
    void recvBody(const std::vector<detail::Fd> &fds, const std::vector<uint16_t> &ports);
    void devBody();
    void drainLost();
    uint32_t gatherLaunch(uint32_t first, uint32_t n, uint8_t *arena);
    void gatherFinish(uint32_t first, uint32_t upto);
    void gatherAll(uint32_t launched, uint32_t n, uint8_t *arena);
    int popEvent(uint8_t **event, size_t *bytes, EventNum_t *eventNum, uint16_t *dataId);
    e2sar_hip_reas_stats deviceStats();
    bool needsUpkeep(const e2sar_hip_reas_stats &st) const;
    void upkeep(const e2sar_hip_reas_stats &st);
    Batch *takeFree();
    Batch *takeFull(bool wait);
    void giveBack(Batch *b);
};

Reassembler::Impl::~Impl()
{
    if (ctx) {
        e2sar_hip_stream_sync(ctx.get(), stream.get());
        e2sar_hip_stream_sync(ctx.get(), copyStream.get());
    }
}

// ctor body: port range and thread/port assignment (cpp:37-181, hpp:308-318)
void Reassembler::Impl::setup(size_t nThreads)
{
    numRecvThreads = nThreads;
    portRange = flags.portRange != -1 ? flags.portRange : get_PortRange((int)nThreads);
    numRecvPorts = (size_t)(portRange > 0 ? 2 << (portRange - 1) : 1);
    if (numRecvThreads > 128) throw E2SARException("Too many reassembly threads requested, limit 128");
    if (numRecvThreads == 0) throw E2SARException("At least one receive thread is required");
    if (portRange < 0 || portRange > 14) throw E2SARException("Port range out of bounds: [0, 14]");
    if (flags.recvStride % 16 || flags.recvStride < 48) throw E2SARException("recvStride must be a multiple of 16, >= 48");
    threadsToPorts.assign(numRecvThreads, {});
    for (size_t i = 0; i < numRecvPorts;)
        for (size_t j = 0; i < numRecvPorts && j < numRecvThreads; i++, j++)
            threadsToPorts[j].push_back((uint16_t)(dataPort + i));
    for (size_t i = 0; i < numRecvPorts; i++) {
        perPortStore.emplace_back(new std::atomic<size_t>(0));
        perPort[(uint16_t)(dataPort + i)] = perPortStore.back().get();
    }

    int rc = detail::make(stream, e2sar_hip_stream_create, flags.gpuDevice);
    if (rc == 0) rc = detail::make(copyStream, e2sar_hip_stream_create, flags.gpuDevice);
    if (rc == 0) rc = detail::make(ctx, e2sar_hip_ctx_create, flags.gpuDevice, stream.get());
    e2sar_hip_reas_config cfg{};
    cfg.withLBHeader = flags.withLBHeader ? 1 : 0;
    cfg.tableSlots = flags.tableSlots;
    cfg.queueCapacity = (uint32_t)std::max<size_t>(4096, flags.recvBatch);
    cfg.lostCapacity = 4096;
    cfg.arenaBytes = flags.arenaBytes;
    cfg.flags = E2SAR_HIP_REAS_COMPACTABLE | (flags.referenceOrder ? E2SAR_HIP_REAS_REFERENCE_ORDER : 0u);
    if (rc == 0) rc = detail::make(reas, e2sar_hip_reas_create, ctx.get(), &cfg);
    for (auto &d : sets) {
        if (rc == 0) rc = detail::alloc_device(ctx.get(), flags.recvBatch * flags.recvStride, d.pkts);
        if (rc == 0) rc = detail::alloc_device(ctx.get(), flags.recvBatch, d.lens);
        if (rc == 0) rc = detail::make(d.h2dDone, e2sar_hip_event_create, ctx.get());
    }
    if (rc == 0) rc = detail::make(gatherDone, e2sar_hip_event_create, ctx.get());
    stageBytes = std::max<size_t>(size_t(64) << 20, 2 * flags.recvBatch * flags.recvStride);
    if (rc == 0) rc = detail::alloc_pinned(stageBytes, stage);
    // host batches: two per receive thread being filled / queued, two on their way to the
    // device, and slack so a receive thread never waits for one while the device thread
    // still holds batches whose copies are done but not yet handed back (MTU 9000 loopback
    // lost datagrams with 4: 0.1 s of waiting for a free batch)
    const size_t nb = 2 * numRecvThreads + 6;
    batches.resize(nb);
    for (auto &b : batches) {
        if (rc == 0) rc = detail::alloc_pinned(flags.recvBatch * flags.recvStride, b.pkts);
        if (rc == 0) rc = detail::alloc_pinned(flags.recvBatch, b.lens);
        freeB.push_back(&b);
    }
    if (rc) throw E2SARException(std::string("Unable to set up the GPU reassembler: ") + e2sar_hip_last_error());
    recs.resize(cfg.queueCapacity);
    lrecs.resize(cfg.lostCapacity);
}

// the one initialiser: the three other constructors delegate to this one
Reassembler::Reassembler(const EjfatURI &uri, const std::string &data_ip, uint16_t starting_port,
                         size_t numRecvThreads, const ReassemblerFlags &rflags)
    : impl(new Impl(uri, rflags, data_ip, starting_port))
{
    impl->setup(numRecvThreads);
}

Reassembler::Reassembler(const EjfatURI &uri, const std::string &data_ip, uint16_t starting_port,
                         std::vector<int> cpuCoreList, const ReassemblerFlags &rflags)
    : Reassembler(uri, data_ip, starting_port, cpuCoreList.size(), rflags) {}

Reassembler::Reassembler(const EjfatURI &uri, uint16_t starting_port, std::vector<int> cpuCoreList,
                         const ReassemblerFlags &rflags, bool v6)
    : Reassembler(uri, std::string(v6 ? "::" : "0.0.0.0"), starting_port, cpuCoreList.size(), rflags) {}

Reassembler::Reassembler(const EjfatURI &uri, uint16_t starting_port, size_t numRecvThreads,
                         const ReassemblerFlags &rflags, bool v6)
    : Reassembler(uri, std::string(v6 ? "::" : "0.0.0.0"), starting_port, numRecvThreads, rflags) {}

Reassembler::~Reassembler() { stopThreads(); }

Reassembler::Impl::Batch *Reassembler::Impl::takeFree()
{
    std::unique_lock<std::mutex> lk(bMu);
    while (freeB.empty() && !stop) bFreeCv.wait_for(lk, std::chrono::milliseconds(10));
    if (freeB.empty()) return nullptr;
    Batch *b = freeB.front();
    freeB.pop_front();
    b->n = 0;
    return b;
}

// E2SAR_RECV_SPIN_US: how long a receive thread stays awake after its last datagram
static uint64_t recv_spin_us()
{
    static const char *const v = getenv("E2SAR_RECV_SPIN_US");
    return v ? (uint64_t)strtoull(v, nullptr, 10) : 200ull;
}

// E2SAR_RECV_PROFILE=1: where the receive and device threads' time goes (stderr at exit).
// lap(bucket) charges the time since start() or the previous lap to `bucket`; report() prints
// the run time and the given fields.  With the profile off, each is only a branch.
struct LapClock {
    const bool on = [] {
        static const bool e = getenv("E2SAR_RECV_PROFILE") != nullptr;
        return e;
    }();
    const uint64_t t0 = on ? detail::now_us() : 0;
    uint64_t last = t0;
    void start() { last = on ? detail::now_us() : 0; }
    void lap(uint64_t &bucket)
    {
        if (!on) return;
        const uint64_t t = detail::now_us();
        bucket += t - last;
        last = t;
    }
    template <class... A> void report(const char *fmt, A... fields) const
    {
        if (on) fprintf(stderr, fmt, (detail::now_us() - t0) * 1e-6, fields...);
    }
};

// The receive loop: select/recvfrom (cpp:293-333) become poll + recvmmsg into a batch.
void Reassembler::Impl::recvBody(const std::vector<detail::Fd> &fds, const std::vector<uint16_t> &ports)
{
    std::vector<pollfd> pf(fds.size());
    for (size_t i = 0; i < fds.size(); i++) pf[i] = pollfd{fds[i].get(), POLLIN, 0};
    const size_t cap = flags.recvBatch;
    const size_t S = flags.recvStride;
    std::vector<mmsghdr> mv(cap);
    std::vector<iovec> iv(cap);
    // the message vector of a batch points at its slots; built once per batch (recvmmsg only
    // writes msg_len / msg_flags back), so a call that returns few datagrams costs no setup
    const Batch *vecFor = nullptr;
    auto vectorFor = [&](const Batch *x) {
        if (vecFor == x) return;
        for (size_t k = 0; k < cap; k++) {
            iv[k].iov_base = x->pkts.get() + k * S;
            iv[k].iov_len = S;
            mv[k].msg_hdr = msghdr{};
            mv[k].msg_hdr.msg_iov = &iv[k];
            mv[k].msg_hdr.msg_iovlen = 1;
        }
        vecFor = x;
    };
    LapClock clk;
    uint64_t tPoll = 0, tRecv = 0, tFree = 0, nCalls = 0, nDg = 0, nFlush = 0, tLastDg = 0;
    const uint64_t spinUs = recv_spin_us();
    uint64_t lastData = 0;
    Batch *b = takeFree();
    uint64_t firstUs = 0;
    auto flush = [&]() {
        if (!b || b->n == 0) return;
        {
            std::lock_guard<std::mutex> lk(bMu);
            fullB.push_back(b);
        }
        bFullCv.notify_one();
        clk.start();
        b = takeFree();
        clk.lap(tFree), nFlush++;
        firstUs = 0;
    };
    while (!stop) {
        if (!b) {
            b = takeFree();
            if (!b) continue;
        }
        const int timeout = (b->n > 0) ? std::max(1, flags.batchTimeout_us / 1000) : 10;   // 10 ms like sleep_tv
        // while datagrams keep coming, stay awake and poll the sockets with non-blocking
        // recvmmsg for up to spinUs after the last one: a sleeping receiver costs the
        // sending side one wakeup per datagram (loopback: half the datagram rate)
        int pr;
        if (lastData && detail::now_us() - lastData < spinUs) {
            for (auto &p : pf) p.revents = POLLIN;
            pr = (int)pf.size();
        } else {
            clk.start();
            pr = poll(pf.data(), pf.size(), timeout);
            clk.lap(tPoll);
        }
        if (pr < 0) {
            if (errno != EINTR) {
                dataErrCnt++;
                lastErrno = errno;
            }
            continue;
        }
        for (size_t i = 0; i < pf.size() && b; i++) {
            if (!(pf[i].revents & POLLIN)) continue;
            while (b && b->n < cap) {
                const size_t room = cap - b->n;
                vectorFor(b);
                mmsghdr *const m = mv.data() + b->n;
                clk.start();
                const int r = recvmmsg(fds[i].get(), m, (unsigned)room, MSG_DONTWAIT, nullptr);
                clk.lap(tRecv), nCalls++;
                if (r > 0) nDg += (uint64_t)r, tLastDg = clk.last - clk.t0;
                if (r < 0) {
                    if (errno != EAGAIN && errno != EWOULDBLOCK && errno != EINTR) {
                        dataErrCnt++;
                        lastErrno = errno;
                    }
                    break;
                }
                for (int k = 0; k < r; k++) {
                    uint32_t len = m[k].msg_len;
                    if (m[k].msg_hdr.msg_flags & MSG_TRUNC) len = (uint32_t)S + 1;   // device: dataErrCnt
                    b->lens[b->n + k] = len;
                }
                perPort[ports[i]]->fetch_add((size_t)r);
                if (r > 0) lastData = detail::now_us();
                if (b->n == 0 && r > 0) firstUs = detail::now_us();
                b->n += (uint32_t)r;
                if (b->n == cap) flush();
                if (r < (int)room) break;
            }
        }
        // (A/B, dropped: flushing a partial batch only while the device thread waits for one
        // lost jumbo datagrams at MTU 9000 -- the batch then grows to 9 MB behind a busy
        // device -- and gained nothing at 1500)
        if (b && b->n > 0 && detail::now_us() - firstUs >= (uint64_t)flags.batchTimeout_us) flush();
    }
    clk.report("recv thread: %.3f s, poll %.3f s, recvmmsg %.3f s (%llu calls, %llu datagrams), "
               "waiting for a free batch %.3f s (%llu batches), last datagram at %.3f s\n",
               tPoll * 1e-6, tRecv * 1e-6, (unsigned long long)nCalls, (unsigned long long)nDg, tFree * 1e-6,
               (unsigned long long)nFlush, tLastDg * 1e-6);
    if (b) {
        {
            std::lock_guard<std::mutex> lk(bMu);
            (b->n ? fullB : freeB).push_back(b);
        }
        bFullCv.notify_one();
    }
}

Reassembler::Impl::Batch *Reassembler::Impl::takeFull(bool wait)
{
    std::unique_lock<std::mutex> lk(bMu);
    if (wait) bFullCv.wait_for(lk, std::chrono::milliseconds(10), [&] { return stop.load() || !fullB.empty(); });
    if (fullB.empty()) return nullptr;
    Batch *b = fullB.front();
    fullB.pop_front();
    return b;
}

void Reassembler::Impl::giveBack(Batch *b)
{
    {
        std::lock_guard<std::mutex> lk(bMu);
        freeB.push_back(b);
    }
    bFreeCv.notify_all();
}

// Completed records recs[first, n) (already polled; their bytes in `arena`) -> pinned
// staging, as many as fit, in one gather launch (e2sar_hip_copy_spans) on the compute
// stream, so it runs ahead of any later kernel or recycle that could overwrite them.
// Returns the index past the last record launched; gatherFinish waits for that launch and
// copies the events into the new[] buffers the caller will own (bin/e2sar_perf.cpp:299).
uint32_t Reassembler::Impl::gatherLaunch(uint32_t first, uint32_t n, uint8_t *arena)
{
    stageOffs.clear();
    std::vector<e2sar_hip_copy_span> spans;
    size_t used = 0;
    uint32_t i = first;
    for (; i < n; i++) {
        const size_t b = recs[i].bytes;
        const size_t need = (b + 63) & ~(size_t)63;
        if (need > stageBytes && i == first) {          // larger than all of the staging: grow it
            e2sar_hip_stream_sync(ctx.get(), stream.get());   // no gather is writing the old one
            stageBytes = 0;
            if (detail::alloc_pinned(need, stage) != 0) {
                lastErr = E2SARErrorc::MemoryError;
                return n;
            }
            stageBytes = need;
        }
        if (used + need > stageBytes) break;
        stageOffs.push_back(used);
        if (b) spans.push_back(e2sar_hip_copy_span{arena + recs[i].arenaOffset, stage.get() + used, b});
        used += need;
    }
    int rc = e2sar_hip_copy_spans(ctx.get(), spans.data(), (uint32_t)spans.size(), stream.get());
    if (rc == 0) rc = e2sar_hip_event_record(ctx.get(), gatherDone.get(), stream.get());
    if (rc) lastErr = E2SARErrorc::SystemError;
    return i;
}

void Reassembler::Impl::gatherFinish(uint32_t first, uint32_t upto)
{
    if (upto <= first) return;
    if (e2sar_hip_event_sync(gatherDone.get()) != 0 || stageOffs.size() != upto - first) {
        lastErr = E2SARErrorc::SystemError;
        return;
    }
    // The reference's eventQueue (hpp:126-127) is a boost::lockfree::queue without
    // fixed_sized: QSIZE only pre-sizes its node pool and push() allocates past it, so an
    // enqueue fails (hpp:138-144 -> enqueueLoss, cpp:413-421) only when allocation does.
    // The queue here is unbounded the same way; a failed allocation is the only loss.
    auto lose = [this](EventNum_t eventNum, uint16_t dataId) {
        hostEnqueueLoss++;
        std::lock_guard<std::mutex> l2(lMu);
        if (lostSeen.insert({eventNum, dataId}).second) lostq.emplace_back(eventNum, dataId, 0);
    };
    std::vector<Ev> ready;
    ready.reserve(upto - first);
    for (uint32_t k = first; k < upto; k++) {
        const auto &r = recs[k];
        std::unique_ptr<uint8_t[]> buf(new (std::nothrow) uint8_t[r.bytes ? r.bytes : 1]);
        if (!buf) {
            lose(r.eventNum, r.dataId);
            continue;
        }
        if (r.bytes) memcpy(buf.get(), stage.get() + stageOffs[k - first], r.bytes);
        ready.push_back(Ev{std::move(buf), r.bytes, r.eventNum, r.dataId});
    }
    {
        std::lock_guard<std::mutex> lk(eMu);
        for (auto &e : ready) {
            try {
                evq.push_back(std::move(e));
            } catch (const std::bad_alloc &) {
                lose(e.eventNum, e.dataId);     // e keeps its buffer, which goes with `ready`
            }
        }
    }
    eCv.notify_all();
}

// Records [0, launched) are in the gather in flight: finish it, then launch and finish
// gathers until all n polled records have left the arena.
void Reassembler::Impl::gatherAll(uint32_t launched, uint32_t n, uint8_t *arena)
{
    gatherFinish(0, launched);
    for (uint32_t done = launched, upto; done < n; done = upto) {
        upto = gatherLaunch(done, n, arena);
        gatherFinish(done, upto);
    }
}

void Reassembler::Impl::drainLost()
{
    uint32_t nl = 0;
    if (e2sar_hip_reas_lost_poll(reas.get(), lrecs.data(), (uint32_t)lrecs.size(), &nl) == 0 && nl) {
        std::lock_guard<std::mutex> l2(lMu);
        for (uint32_t i = 0; i < nl; i++) {   // logLostEvent dedupe (hpp:266-269)
            const auto &l = lrecs[i];
            if (lostSeen.insert({l.eventNum, l.dataId}).second) lostq.emplace_back(l.eventNum, l.dataId, l.numFragments);
        }
    }
}

// Recycle or compact once the arena or the table is half used.  Completed and timed-out
// slots keep their table entries until then, so with small events and a steady stream
// the table fills long before the arena; compaction keeps only the events in progress.
// It is skipped when it would not free at least half of the table (most slots live).
// Runs with the device idle and every completed record polled and gathered.
bool Reassembler::Impl::needsUpkeep(const e2sar_hip_reas_stats &st) const
{
    if (st.completedPending != 0) return false;
    const bool arenaHalf = st.arenaUsed > flags.arenaBytes / 2;
    const bool tableHalf = st.tableUsed > flags.tableSlots / 2 &&
                           st.tableUsed > 2 * (uint64_t)std::max<int64_t>(st.inProgress, 0);
    return arenaHalf || tableHalf;
}

void Reassembler::Impl::upkeep(const e2sar_hip_reas_stats &st)
{
    const int rc = st.inProgress == 0 ? e2sar_hip_reas_recycle(reas.get(), 0, nullptr) : e2sar_hip_reas_compact(reas.get(), nullptr);
    if (rc) lastErr = static_cast<E2SARErrorc>(-rc);
    else upkeeps++;
}

// The device thread.  Per batch b (two device buffers, sets[b % 2]):
//   copy b+1 in (copy stream, beside kernel b) -> poll b (waits for kernel b and the copy)
//   -> hand b+1's host batch back -> stats (device idle) -> gather b's events (compute
//   stream) -> [GC pass / recycle / compact, before any later kernel] -> kernel b+1
//   (after the copy's event) -> host copies of b's events while kernel b+1 runs.
void Reassembler::Impl::devBody()
{
    uint64_t lastGc = detail::steady_ms();
    const uint32_t stride = (uint32_t)flags.recvStride;
    bool kernelInFlight = false;       // a launched batch whose results are not yet drained
    int cur = 0;                       // device set of the next copy
    e2sar_hip_ctx *const c = ctx.get();
    e2sar_hip_reas *const r = reas.get();
    LapClock clk;
    uint64_t pWait = 0, pPoll = 0, pGather = 0, pUpkeep = 0, pLaunch = 0, pCycles = 0, pBatches = 0, pDg = 0, pEvents = 0,
             pLastEv = 0;
    while (true) {
        clk.start();
        Batch *b = takeFull(!kernelInFlight);
        clk.lap(pWait), pCycles++, pBatches += b ? 1 : 0, pDg += b ? b->n : 0;
        if (!b && !kernelInFlight && stop && recvActive.load() == 0) {
            std::lock_guard<std::mutex> lk(bMu);
            if (fullB.empty()) break;
        }
        DevSet &d = sets[cur];
        uint32_t bn = 0;
        uint64_t bnow = 0;
        if (b) {
            bn = b->n;
            bnow = detail::steady_ms();
            int rc = e2sar_hip_memcpy_async(c, d.pkts.get(), b->pkts.get(), (size_t)b->n * stride, 0, copyStream.get());
            if (rc == 0) rc = e2sar_hip_memcpy_async(c, d.lens.get(), b->lens.get(), (size_t)b->n * 4, 0, copyStream.get());
            if (rc == 0) rc = e2sar_hip_event_record(c, d.h2dDone.get(), copyStream.get());
            if (rc) lastErr = static_cast<E2SARErrorc>(-rc);
        }
        uint32_t n = 0;
        clk.start();
        if (e2sar_hip_reas_poll(r, recs.data(), (uint32_t)recs.size(), &n) != 0) lastErr = E2SARErrorc::SystemError;
        clk.lap(pPoll), pEvents += n;
        if (n) pLastEv = clk.last - clk.t0;
        if (b) giveBack(b);                                   // its bytes are on the device now
        kernelInFlight = false;
        e2sar_hip_reas_stats st{};
        const bool haveStats = e2sar_hip_reas_get_stats(r, &st) == 0;
        if (haveStats) {
            std::lock_guard<std::mutex> lk(sMu);
            lastStats = st;
        }
        uint8_t *arena = e2sar_hip_reas_arena(r);
        const uint32_t launched = n ? gatherLaunch(0, n, arena) : 0;
        const uint64_t now = detail::steady_ms();
        const bool gcDue = now - lastGc >= (uint64_t)flags.eventTimeout_ms;
        const bool upkeepDue = haveStats && needsUpkeep(st);
        bool gathered = n == 0;
        clk.start();
        if (gcDue || upkeepDue) {
            // every completed event leaves the arena before the GC pass, a recycle or a compaction
            gatherAll(launched, n, arena);
            gathered = true;
            if (gcDue) {                              // GC thread period (cpp:252-283)
                e2sar_hip_reas_gc(r, now, (uint64_t)flags.eventTimeout_ms, nullptr);
                lastGc = now;
                drainLost();
            }
            if (upkeepDue) upkeep(st);
        }
        clk.lap(pUpkeep);
        if (b) {
            int rc = e2sar_hip_stream_wait_event(c, nullptr, d.h2dDone.get());
            if (rc == 0) rc = e2sar_hip_reassemble_batch(r, d.pkts.get(), stride, d.lens.get(), bn, bnow, nullptr);
            if (rc) lastErr = static_cast<E2SARErrorc>(-rc);
            else kernelInFlight = true;
            cur ^= 1;
        }
        clk.lap(pLaunch);
        if (!gathered) gatherAll(launched, n, arena);          // while that kernel runs
        clk.lap(pGather);
    }
    clk.report("device thread: %.3f s, %llu cycles (%llu batches, %llu datagrams, %llu events), waiting %.3f s, "
               "poll %.3f s, upkeep/GC %.3f s, copy+launch %.3f s, gather %.3f s, last event at %.3f s\n",
               (unsigned long long)pCycles, (unsigned long long)pBatches, (unsigned long long)pDg,
               (unsigned long long)pEvents, pWait * 1e-6, pPoll * 1e-6, pUpkeep * 1e-6, pLaunch * 1e-6, pGather * 1e-6,
               pLastEv * 1e-6);
    uint32_t n = 0;
    if (e2sar_hip_reas_poll(r, recs.data(), (uint32_t)recs.size(), &n) == 0 && n) gatherAll(0, n, e2sar_hip_reas_arena(r));
    drainLost();
}

result<int> Reassembler::registerWorker(const std::string &) noexcept
{
    if (impl->flags.useCP) return E2SARErrorInfo{E2SARErrorc::LogicError, "no control plane on this data path"};
    return 0;   // cpp:603-612 with useCP == false
}

result<int> Reassembler::deregisterWorker() noexcept { return 0; }

// cpp:184-234 and socket open cpp:435-510
result<int> Reassembler::openAndStart() noexcept
{
    auto &m = *impl;
    if (m.started) return 0;
    std::vector<std::vector<detail::Fd>> tfds(m.numRecvThreads);   // closed on every early return
    for (size_t t = 0; t < m.numRecvThreads; t++) {
        for (uint16_t port : m.threadsToPorts[t]) {
            const auto addr = detail::sock_addr(m.dataIP, port, m.v6);
            if (!addr.ok) return E2SARErrorInfo{E2SARErrorc::ParameterError, "bad data address " + m.dataIP};
            detail::Fd fd(socket(m.v6 ? AF_INET6 : AF_INET, SOCK_DGRAM, 0));
            if (!fd.valid()) return E2SARErrorInfo{E2SARErrorc::SocketError, strerror(errno)};
            setsockopt(fd.get(), SOL_SOCKET, SO_RCVBUF, &m.flags.rcvSocketBufSize, sizeof(int));
            const int one = 1;
            setsockopt(fd.get(), SOL_SOCKET, SO_REUSEADDR, &one, sizeof(one));
            if (bind(fd.get(), addr.sa(), addr.len) != 0) {
                const std::string err = strerror(errno);
                return E2SARErrorInfo{E2SARErrorc::SocketError, "bind port " + std::to_string(port) + ": " + err};
            }
            tfds[t].push_back(std::move(fd));
        }
    }
    m.stop = false;
    m.recvActive = (int)m.numRecvThreads;
    for (size_t t = 0; t < m.numRecvThreads; t++)
        m.recvThreads.emplace_back([&m, t, fds = std::move(tfds[t])]() mutable {
            m.recvBody(fds, m.threadsToPorts[t]);
            fds.clear();                // the sockets close before the device thread hears of it
            m.recvActive--;
            m.bFullCv.notify_one();
        });
    m.devThread = std::thread([&m] { m.devBody(); });
    m.started = true;
    return 0;
}

// the front of the event queue (eMu held), its buffer handed to the caller; -1 when empty
int Reassembler::Impl::popEvent(uint8_t **event, size_t *bytes, EventNum_t *eventNum, uint16_t *dataId)
{
    if (evq.empty()) return -1;
    Ev &e = evq.front();
    *event = e.event.release();
    *bytes = e.bytes;
    *eventNum = e.eventNum;
    *dataId = e.dataId;
    evq.pop_front();
    return 0;
}

// cpp:626-641
result<int> Reassembler::getEvent(uint8_t **event, size_t *bytes, EventNum_t *eventNum, uint16_t *dataId) noexcept
{
    std::lock_guard<std::mutex> lk(impl->eMu);
    return impl->popEvent(event, bytes, eventNum, dataId);
}

// cpp:643-676: wait in 10 ms slices; wait_ms == 0 waits until stopThreads()
result<int> Reassembler::recvEvent(uint8_t **event, size_t *bytes, EventNum_t *eventNum, uint16_t *dataId,
                                   uint64_t wait_ms) noexcept
{
    auto &m = *impl;
    const auto t0 = std::chrono::steady_clock::now();
    std::unique_lock<std::mutex> lk(m.eMu);
    while (m.evq.empty()) {
        if (m.stop) return -1;
        m.eCv.wait_for(lk, std::chrono::milliseconds(10));
        if (wait_ms && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(wait_ms) && m.evq.empty())
            return -1;
    }
    return m.popEvent(event, bytes, eventNum, dataId);
}

// the device's counters: live once started, else (or on failure) the device thread's last copy
e2sar_hip_reas_stats Reassembler::Impl::deviceStats()
{
    e2sar_hip_reas_stats st{};
    if (!started || e2sar_hip_reas_get_stats(reas.get(), &st) != 0) {
        std::lock_guard<std::mutex> lk(sMu);
        st = lastStats;
    }
    return st;
}

const Reassembler::ReportedStats Reassembler::getStats() const noexcept
{
    auto &m = *impl;
    const e2sar_hip_reas_stats st = m.deviceStats();
    ReportedStats r{};
    r.enqueueLoss = st.enqueueLoss + m.hostEnqueueLoss.load();
    r.reassemblyLoss = st.reassemblyLoss;
    r.eventSuccess = st.eventSuccess;
    r.lastErrno = m.lastErrno.load();
    r.grpcErrCnt = 0;
    r.dataErrCnt = m.dataErrCnt.load() + (int)st.dataErrCnt;
    r.lastE2SARError = m.lastErr.load();
    r.totalPackets = st.totalPackets;
    r.totalBytes = st.totalBytes;
    r.badHeaderDiscards = st.badHeaderDiscards;
    return r;
}

result<std::tuple<EventNum_t, uint16_t, size_t>> Reassembler::get_LostEvent() noexcept
{
    auto &m = *impl;
    std::lock_guard<std::mutex> lk(m.lMu);
    if (m.lostq.empty()) return E2SARErrorInfo{E2SARErrorc::NotFound, "Lost event queue is empty"};
    auto t = m.lostq.front();
    m.lostq.pop_front();
    return t;
}

result<std::list<std::pair<uint16_t, size_t>>> Reassembler::get_FDStats() noexcept
{
    auto &m = *impl;
    if (!m.stop) return E2SARErrorInfo{E2SARErrorc::LogicError, "This method should only be called after the threads have been stopped."};
    std::list<std::pair<uint16_t, size_t>> out;
    for (auto &kv : m.perPort) out.emplace_back(kv.first, kv.second->load());
    return out;
}

size_t Reassembler::get_numRecvThreads() const noexcept { return impl->numRecvThreads; }
const std::pair<int, int> Reassembler::get_recvPorts() const noexcept
{
    return std::make_pair((int)impl->dataPort, (int)(impl->dataPort + impl->numRecvPorts - 1));
}
int Reassembler::get_portRange() const noexcept { return impl->portRange; }
const std::string Reassembler::get_dataIP() const noexcept { return impl->dataIP; }

const Reassembler::DeviceStats Reassembler::getDeviceStats() const noexcept
{
    auto &m = *impl;
    const e2sar_hip_reas_stats st = m.deviceStats();
    return DeviceStats{st.tableUsed, st.arenaUsed, m.upkeeps.load(), st.inProgress, st.errorFlags};
}

void Reassembler::stopThreads()
{
    auto &m = *impl;
    if (m.stop && !m.started) return;
    m.stop = true;
    m.eCv.notify_all();
    m.bFreeCv.notify_all();
    for (auto &t : m.recvThreads)
        if (t.joinable()) t.join();
    m.bFullCv.notify_all();
    if (m.devThread.joinable()) m.devThread.join();
    m.started = false;
}

}  // namespace e2sar
