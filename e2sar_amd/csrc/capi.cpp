// capi.cpp -- the extern "C" boundary declared in include/e2sar_hip.h.
//
// Host-side glue only: argument checks (mirroring the reference's sanity checks),
// device allocation of the reassembly state, and the hand-off of device records to
// the caller.  Every byte of event or datagram data is moved by the kernels of
// sar_kernels.hip (its device headers); there is no CPU fallback.
#ifndef E2SAR_HIP_EXPERIMENTAL
#define E2SAR_HIP_EXPERIMENTAL 0
#endif
#if E2SAR_HIP_EXPERIMENTAL
#include "e2sar_hip_experimental.h"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <set>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "e2sar_hip.h"
#include "rows_div.hpp"
#include "sar_kernels.hpp"

using namespace e2sar_amd;

namespace {

thread_local std::string g_lastError;

int fail(int code, const std::string &msg)
{
    g_lastError = msg;
    return code;
}

int hip_fail(hipError_t e, const char *what)
{
    return fail(E2SAR_HIP_ERR_SYSTEM, std::string(what) + ": " + hipGetErrorString(e));
}

// A device allocation the runtime refused, as "<what>: <error>".  The runtime also keeps the
// error as the thread's last one, where the hipGetLastError of the next launcher (or of any
// other user of the runtime in this process) would find it: reported here, so cleared here.
int alloc_fail(hipError_t e, const char *what)
{
    (void)hipGetLastError();
    return fail(E2SAR_HIP_ERR_MEMORY, std::string(what) + ": " + hipGetErrorString(e));
}

#define HIP_TRY(expr)                                   \
    do {                                                \
        hipError_t _e = (expr);                         \
        if (_e != hipSuccess) return hip_fail(_e, #expr); \
    } while (0)

}  // namespace

// A context is shared: every reassembler created on it holds a reference, so the caller may
// destroy the context and its reassemblers in any order (a garbage collector tearing down a
// reference cycle picks one) -- the memory goes with the last reference.
struct e2sar_hip_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::atomic<int> refs{1};
};
static void ctx_release(e2sar_hip_ctx *c)
{
    if (c && c->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete c;
}

/* ---------------- owners ---------------- */

// What this file allocates is held by a move-only owner: outside the public free / destroy
// entry points, these deleters are the only hipFree, hipEventDestroy and reference drop.
namespace {

template <auto Destroy> struct Deleter {
    template <class T> void operator()(T *p) const { (void)Destroy(p); }
};
using DevMem = std::unique_ptr<void, Deleter<hipFree>>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Deleter<hipEventDestroy>>;
using CtxRef = std::unique_ptr<e2sar_hip_ctx, Deleter<ctx_release>>;     // adopts a reference already taken
static_assert(!std::is_copy_constructible_v<DevMem> && !std::is_copy_constructible_v<Event> &&
                  !std::is_copy_constructible_v<CtxRef>,
              "owners move, they do not copy");

// hipMalloc into an owner; a failure leaves it empty
hipError_t dev_alloc(DevMem &m, size_t bytes)
{
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    m.reset(e == hipSuccess ? p : nullptr);
    return e;
}

// An internal buffer that grows (grow()): the allocation and its size
struct GrowBuf {
    DevMem mem;
    size_t bytes = 0;
};

}  // namespace

// The order in which a reassembler's memory goes is the reverse of the declarations below:
// the destructor waits for the device, then the event, the retired buffers, the per-stream
// scratch, both arenas, the turn's move list, the alternate table and the state block are
// released, and the reference on the context last.
struct e2sar_hip_reas {
    CtxRef ctx;                      // first, so destroyed last: the destructor sets its device
    e2sar_hip_reas_config cfg{};
    // views into the memory below; compaction swaps the slots and arena of the two
    ReasDev dev{};
    ReasDev alt{};                   // second slots + arena (COMPACTABLE), same ctl/lists
    DevMem state;                    // slots | ctl | shards | occupancy shards | completed | lost
    DevMem altSlots;
    DevMem turnMoves;                // the turn's move list (COMPACTABLE): kTurnMoveBytes per table slot
    DevMem arena[2];                 // owned by identity, whichever of dev / alt points at which
    // Internal buffers, one set PER STREAM (two batches launched on different streams must
    // not share work records or ready counters while both run): the reference-order sort
    // keys / records / sort storage, the PktInfo/FinishRec work buffer of reassemble_batch
    // (reference order, or batches above kFusedMaxBytes), the chained form's ready counters.
    // They grow on demand, never inside a graph capture, and a buffer they outgrow is kept
    // (retired) while a graph captured before the growth may still hold its address.
    struct Scratch {
        GrowBuf ro;
        // a reference-order launch sequence failed part way: the key pass may have left run
        // counts that only the place / walk kernels reset, so the next batch re-zeroes them
        bool roDirty = false;
        GrowBuf work;
        GrowBuf tiles;
    };
    std::map<hipStream_t, Scratch> scratch;
    std::vector<DevMem> retired;
    // the streams launched on outside capture: poll / lost_poll / get_stats wait for those
    // streams only, not for the whole device (an event recorded on each at snapshot time --
    // not after every launch: a marker between kernels lengthens the next kernel's start)
    std::set<hipStream_t> streams;
    Event waitEv;
    bool sawCapture = false;         // a launch was captured into a graph: snapshots wait for the device
    std::mutex mu;

    e2sar_hip_reas(e2sar_hip_ctx *c, const e2sar_hip_reas_config &config) : ctx(c), cfg(config)
    {
        c->refs.fetch_add(1, std::memory_order_relaxed);
    }
    ~e2sar_hip_reas()
    {
        (void)hipSetDevice(ctx->device);
        // launches on any stream (the caller's, a graph replay's) may still use the table, the
        // arena and the internal buffers: wait for the device before the members free them
        (void)hipDeviceSynchronize();
    }
};

static bool ref_order(const e2sar_hip_reas *r) { return (r->cfg.flags & E2SAR_HIP_REAS_REFERENCE_ORDER) != 0; }

static hipStream_t stream_of(const e2sar_hip_ctx *ctx, void *stream)
{
    return stream ? static_cast<hipStream_t>(stream) : ctx->stream;
}

static bool capturing(hipStream_t s)
{
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
}

// After a launch through this reassembler on stream s (caller holds r->mu): remember the
// stream, so a later snapshot waits for exactly the streams this reassembler used.
static void note_launch(e2sar_hip_reas *r, hipStream_t s)
{
    if (capturing(s)) r->sawCapture = true;          // replays run wherever the caller puts them
    else r->streams.insert(s);
}

// The prologue and epilogue of a call on a context: ctx must not be NULL; on its device and
// (stream == NULL) its default stream run body(s).  body returns the call's hipError_t,
// reported as "<what>: <error>", or, where it can fail in other ways or words, an ABI code
// with the message already set.  An entry point with argument checks says "ctx is NULL"
// itself before them: the device is set last.
template <typename Body>
static int ctx_call(const e2sar_hip_ctx *ctx, void *stream, const char *what, Body body)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = stream_of(ctx, stream);
    if constexpr (std::is_same_v<decltype(body(s)), hipError_t>) {
        const hipError_t e = body(s);
        return e == hipSuccess ? E2SAR_HIP_OK : hip_fail(e, what);
    } else {
        return body(s);
    }
}

// The prologue and epilogue of every launch through a reassembler: r must not be NULL; under
// r->mu, a ctx_call on r's context -- or on `on`, where the caller names another context --
// that runs body(s), then remembers the stream (note_launch).
template <typename Body>
static int reas_launch(e2sar_hip_reas *r, void *stream, const char *what, Body body, const e2sar_hip_ctx *on = nullptr)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    std::lock_guard<std::mutex> lk(r->mu);
    if (!on) on = r->ctx.get();
    const int rc = ctx_call(on, stream, what, body);
    if (rc == E2SAR_HIP_OK) note_launch(r, stream_of(on, stream));
    return rc;
}

/* ---------------- argument checks shared by the entry points ---------------- */

// nPackets datagram slots at d_packets, whatever reads them: alignment, and 16-byte words a
// 32-bit index can count
static int check_packets(const uint8_t *d_packets, uint32_t stride, uint32_t nPackets)
{
    if (((uintptr_t)d_packets & 15u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "packet buffer not 16-byte aligned");
    if ((uint64_t)nPackets * (stride >> 4) > 0xFFFFFFFFull) return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "batch too large");
    return E2SAR_HIP_OK;
}

// A batch of nPackets datagram slots of `stride` bytes at d_packets for a reassembly, with or
// without LB headers: the slot stride, then check_packets.
static int check_slots(bool withLB, const uint8_t *d_packets, uint32_t stride, uint32_t nPackets)
{
    const uint32_t hl = withLB ? E2SAR_HIP_LBRE_HDR_LEN : E2SAR_HIP_RE_HDR_LEN;
    if ((stride & 15u) || stride < hl + 16u) return fail(E2SAR_HIP_ERR_PARAMETER, "stride must be a multiple of 16 and > header + 16");
    return check_packets(d_packets, stride, nPackets);
}
static int check_batch(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride, uint32_t nPackets)
{
    return check_slots(r->cfg.withLBHeader != 0, d_packets, stride, nPackets);
}

// The caller's work buffer of a classified batch of n datagrams; tooSmall is the entry
// point's own wording of that failure.
static int check_work(const void *d_work, size_t workBytes, uint32_t n, const char *tooSmall)
{
    if (((uintptr_t)d_work & 255u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "work buffer not 256-byte aligned");
    if (workBytes < work_bytes(n)) return fail(E2SAR_HIP_ERR_PARAMETER, tooSmall);
    return E2SAR_HIP_OK;
}

// The datagram layout a segmentation writes: maxPldLen (udpBound: at most a UDP datagram's),
// the slot stride, the packet buffer's alignment (a NULL buffer passes: its caller checks).
static int check_seg_layout(uint32_t maxPldLen, uint32_t stride, const uint8_t *d_packets, bool udpBound = true)
{
    if (maxPldLen == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "maxPldLen is 0 (MTU too small)");
    if (udpBound && maxPldLen > 65535u) return fail(E2SAR_HIP_ERR_PARAMETER, "maxPldLen above a UDP datagram");
    if ((stride & 15u) || stride < E2SAR_HIP_LBRE_HDR_LEN + maxPldLen)
        return fail(E2SAR_HIP_ERR_PARAMETER, "stride must be a multiple of 16 and hold 36 + maxPldLen");
    if (((uintptr_t)d_packets & 15u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "packet buffer not 16-byte aligned");
    return E2SAR_HIP_OK;
}

static int check_world(uint32_t world, uint32_t self)
{
    if (world == 0 || world > 64 || self >= world) return fail(E2SAR_HIP_ERR_PARAMETER, "world must be 1..64, self < world");
    return E2SAR_HIP_OK;
}

// What every routing form checks first, in this order: the context, the ranks, the slot stride.
static int check_route(const e2sar_hip_ctx *ctx, uint32_t world, uint32_t self, uint32_t stride)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (int rc = check_world(world, self)) return rc;
    if ((stride & 15u) || stride < 48u) return fail(E2SAR_HIP_ERR_PARAMETER, "stride must be a multiple of 16, >= 48");
    return E2SAR_HIP_OK;
}

// Where collect and build pack events: the output buffer's alignment; and the pitch of its
// rows or cells and the alignment of its ragged events, `align` 0 becoming the default.  Two
// checks, since the two entry points refuse in different orders.
static int check_pack_out(const uint8_t *d_out)
{
    if (((uintptr_t)d_out & 255u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "output buffer not 256-byte aligned");
    return E2SAR_HIP_OK;
}
static int check_pack_layout(uint32_t pitch, uint32_t &align)
{
    if (pitch & 15u) return fail(E2SAR_HIP_ERR_PARAMETER, "pitch must be a multiple of 16");
    if (align == 0) align = 256;
    if (align < 16 || align > 4096 || (align & (align - 1)))
        return fail(E2SAR_HIP_ERR_PARAMETER, "align must be 0 or a power of two in [16, 4096]");
    return E2SAR_HIP_OK;
}

// reassemble_batch keeps the fused kernel up to this many bytes of datagram slots (a batch
// that can still sit in the 256 MiB Infinity Cache) and switches to the split form above
static constexpr uint64_t kFusedMaxBytes = 320ull << 20;

// Streaming (non-temporal) datagram loads in the scatter: for datagrams the caller declares
// cold (E2SAR_HIP_REAS_COLD_DATAGRAMS), and for a batch too large to still be cached.
static bool cold_loads(const e2sar_hip_reas *r, uint32_t n, uint32_t stride)
{
    return (r->cfg.flags & E2SAR_HIP_REAS_COLD_DATAGRAMS) != 0 || (uint64_t)n * stride > kFusedMaxBytes;
}

// Grow an internal buffer of stream s to at least `need` bytes (a quarter more, to
// amortise); caller holds r->mu.  The old buffer is retired, not freed: kernels of earlier
// batches may still read it, and a graph captured earlier holds its address.  Inside a
// capture a buffer cannot grow (allocation there would break the capture): the call fails
// with a LogicError naming the remedy instead.
static int grow(e2sar_hip_reas *r, hipStream_t s, GrowBuf &b, size_t need, bool *grew = nullptr)
{
    if (grew) *grew = false;
    if (need <= b.bytes) return E2SAR_HIP_OK;
    if (capturing(s))
        return fail(E2SAR_HIP_ERR_LOGIC, "an internal buffer must grow for this batch size inside a graph capture: "
                                         "run one batch of the largest size on this stream before capturing");
    const size_t want = need + need / 4;
    DevMem nb;
    const hipError_t e = dev_alloc(nb, want);
    if (e != hipSuccess) return alloc_fail(e, "hipMalloc(internal buffer)");
    if (b.mem) r->retired.push_back(std::move(b.mem));
    b.mem = std::move(nb);
    b.bytes = want;
    if (grew) *grew = true;
    return E2SAR_HIP_OK;
}

// Free the internal buffers of stream s (caller holds r->mu and knows none of its launches
// still runs).  Buffers a graph capture may hold are retired instead, as in grow().
static void drop_scratch(e2sar_hip_reas *r, hipStream_t s)
{
    auto it = r->scratch.find(s);
    if (it == r->scratch.end()) return;
    if (r->sawCapture)
        for (GrowBuf *b : {&it->second.ro, &it->second.work, &it->second.tiles})
            if (b->mem) r->retired.push_back(std::move(b->mem));
    r->scratch.erase(it);
}

extern "C" {

int e2sar_hip_abi_version(void) { return E2SAR_HIP_ABI_VERSION; }

const char *e2sar_hip_last_error(void) { return g_lastError.c_str(); }

int e2sar_hip_ctx_create(int device, void *stream, e2sar_hip_ctx **out)
{
    if (!out) return fail(E2SAR_HIP_ERR_PARAMETER, "out is NULL");
    int n = 0;
    HIP_TRY(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return fail(E2SAR_HIP_ERR_PARAMETER, "no such device");
    HIP_TRY(hipSetDevice(device));
    auto *c = new e2sar_hip_ctx;
    c->device = device;
    c->stream = static_cast<hipStream_t>(stream);   // NULL = the device's default stream
    *out = c;
    return E2SAR_HIP_OK;
}

void e2sar_hip_ctx_destroy(e2sar_hip_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx_release(ctx);
}

int e2sar_hip_stream_create(int device, void **out)
{
    if (!out) return fail(E2SAR_HIP_ERR_PARAMETER, "out is NULL");
    HIP_TRY(hipSetDevice(device));
    hipStream_t s = nullptr;
    HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    *out = s;
    return E2SAR_HIP_OK;
}

int e2sar_hip_stream_destroy(void *stream)
{
    if (!stream) return E2SAR_HIP_OK;
    HIP_TRY(hipStreamDestroy(static_cast<hipStream_t>(stream)));
    return E2SAR_HIP_OK;
}

void *e2sar_hip_ctx_stream(e2sar_hip_ctx *ctx) { return ctx ? ctx->stream : nullptr; }
int e2sar_hip_ctx_device(e2sar_hip_ctx *ctx) { return ctx ? ctx->device : -1; }

int e2sar_hip_ctx_sync(e2sar_hip_ctx *ctx)
{
    return ctx_call(ctx, nullptr, "hipStreamSynchronize(ctx->stream)", [](hipStream_t s) { return hipStreamSynchronize(s); });
}

int e2sar_hip_device_alloc(e2sar_hip_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    return ctx_call(ctx, nullptr, "hipMalloc", [&](hipStream_t) -> int {
        const hipError_t e = hipMalloc(out, bytes ? bytes : 1);
        return e == hipSuccess ? E2SAR_HIP_OK : alloc_fail(e, "hipMalloc");
    });
}

int e2sar_hip_device_free(e2sar_hip_ctx *ctx, void *p)
{
    return ctx_call(ctx, nullptr, "hipFree(p)", [&](hipStream_t) { return hipFree(p); });
}

int e2sar_hip_host_alloc(size_t bytes, void **out)
{
    if (!out) return fail(E2SAR_HIP_ERR_PARAMETER, "out is NULL");
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return fail(E2SAR_HIP_ERR_MEMORY, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    return E2SAR_HIP_OK;
}

int e2sar_hip_host_free(void *p)
{
    HIP_TRY(hipHostFree(p));
    return E2SAR_HIP_OK;
}

// dst <- src on the context's stream, finished on return
static int memcpy_sync(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes, hipMemcpyKind kind)
{
    return ctx_call(ctx, nullptr, "memcpy", [&](hipStream_t s) -> int {
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, s));
        HIP_TRY(hipStreamSynchronize(s));
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_memcpy_h2d(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    return memcpy_sync(ctx, dst, src, bytes, hipMemcpyHostToDevice);
}

int e2sar_hip_memcpy_d2h(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes)
{
    return memcpy_sync(ctx, dst, src, bytes, hipMemcpyDeviceToHost);
}

int e2sar_hip_memset_async(e2sar_hip_ctx *ctx, void *dst, int value, size_t bytes, void *stream)
{
    // a fill kernel, not hipMemsetAsync: the call may be captured into a HIP graph, where
    // memset nodes misbehave on replay
    return ctx_call(ctx, stream, "launch_fill_bytes", [&](hipStream_t s) { return launch_fill_bytes(dst, value, bytes, s); });
}

int e2sar_hip_memset_d(e2sar_hip_ctx *ctx, void *dst, int value, size_t bytes)
{
    return e2sar_hip_memset_async(ctx, dst, value, bytes, nullptr);
}

int e2sar_hip_memcpy_async(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes, int kind, void *stream)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (kind < 0 || kind > 2) return fail(E2SAR_HIP_ERR_PARAMETER, "kind must be 0 (H2D), 1 (D2H) or 2 (D2D)");
    if (bytes == 0) return E2SAR_HIP_OK;
    const hipMemcpyKind k = kind == 0 ? hipMemcpyHostToDevice : kind == 1 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    return ctx_call(ctx, stream, "hipMemcpyAsync(dst, src, bytes, k, s)",
                    [&](hipStream_t s) { return hipMemcpyAsync(dst, src, bytes, k, s); });
}

int e2sar_hip_stream_sync(e2sar_hip_ctx *ctx, void *stream)
{
    return ctx_call(ctx, stream, "hipStreamSynchronize", [](hipStream_t s) { return hipStreamSynchronize(s); });
}

int e2sar_hip_event_create(e2sar_hip_ctx *ctx, void **out)
{
    if (!ctx || !out) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    return ctx_call(ctx, nullptr, "event_create", [&](hipStream_t) -> int {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *out = e;
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_event_destroy(void *event)
{
    if (event) HIP_TRY(hipEventDestroy(static_cast<hipEvent_t>(event)));
    return E2SAR_HIP_OK;
}

int e2sar_hip_event_record(e2sar_hip_ctx *ctx, void *event, void *stream)
{
    if (!ctx || !event) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    HIP_TRY(hipEventRecord(static_cast<hipEvent_t>(event), stream_of(ctx, stream)));
    return E2SAR_HIP_OK;
}

int e2sar_hip_stream_wait_event(e2sar_hip_ctx *ctx, void *stream, void *event)
{
    if (!ctx || !event) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    HIP_TRY(hipStreamWaitEvent(stream_of(ctx, stream), static_cast<hipEvent_t>(event), 0));
    return E2SAR_HIP_OK;
}

int e2sar_hip_event_query(void *event)
{
    if (!event) return fail(E2SAR_HIP_ERR_PARAMETER, "event is NULL");
    const hipError_t e = hipEventQuery(static_cast<hipEvent_t>(event));
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return hip_fail(e, "hipEventQuery");
}

int e2sar_hip_event_sync(void *event)
{
    if (!event) return fail(E2SAR_HIP_ERR_PARAMETER, "event is NULL");
    HIP_TRY(hipEventSynchronize(static_cast<hipEvent_t>(event)));
    return E2SAR_HIP_OK;
}

int e2sar_hip_copy_spans(e2sar_hip_ctx *ctx, const e2sar_hip_copy_span *spans, uint32_t n, void *stream)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (n == 0) return E2SAR_HIP_OK;
    if (!spans) return fail(E2SAR_HIP_ERR_PARAMETER, "spans is NULL");
    return ctx_call(ctx, stream, "copy_spans launch", [&](hipStream_t s) -> int {
        for (uint32_t i0 = 0; i0 < n; i0 += kCopySpansPerLaunch) {
            CopySpans cs{};
            cs.n = std::min<uint32_t>(kCopySpansPerLaunch, n - i0);
            uint64_t most = 0;
            for (uint32_t k = 0; k < cs.n; k++) {
                const auto &sp = spans[i0 + k];
                if (sp.bytes && (!sp.src || !sp.dst)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL span pointer");
                cs.s[k] = CopySpan{reinterpret_cast<uint64_t>(sp.src), reinterpret_cast<uint64_t>(sp.dst), sp.bytes};
                most = std::max<uint64_t>(most, sp.bytes);
            }
            const hipError_t e = launch_copy_spans(cs, most, s);
            if (e != hipSuccess) return hip_fail(e, "copy_spans launch");
        }
        return E2SAR_HIP_OK;
    });
}

/* ---------------- geometry ---------------- */

size_t e2sar_hip_total_hdr_len(int useIPv6)
{
    return (useIPv6 ? 40u : 20u) + 8u + E2SAR_HIP_LB_HDR_LEN + E2SAR_HIP_RE_HDR_LEN;
}

size_t e2sar_hip_max_pld_len(uint32_t mtu, int useIPv6)
{
    const size_t h = e2sar_hip_total_hdr_len(useIPv6);
    return mtu > h ? mtu - h : 0;
}

size_t e2sar_hip_num_packets(size_t bytes, size_t maxPldLen)
{
    return maxPldLen ? (bytes + maxPldLen - 1) / maxPldLen : 0;
}

uint32_t e2sar_hip_packet_stride(size_t maxPldLen)
{
    return (uint32_t)((E2SAR_HIP_LBRE_HDR_LEN + maxPldLen + 15) & ~(size_t)15);
}

/* ---------------- segmentation ---------------- */

int e2sar_hip_seg_plan(e2sar_hip_seg_event *events, uint32_t nEvents, size_t maxPldLen,
                       uint32_t *totalPackets, uint32_t *maxPacketsPerEvent)
{
    if (!events && nEvents) return fail(E2SAR_HIP_ERR_PARAMETER, "events is NULL");
    if (maxPldLen == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "maxPldLen is 0 (MTU too small)");
    uint64_t total = 0;
    uint32_t mx = 0;
    for (uint32_t i = 0; i < nEvents; i++) {
        const uint64_t n = e2sar_hip_num_packets(events[i].bytes, maxPldLen);
        events[i].pktBase = (uint32_t)total;
        total += n;
        mx = std::max<uint32_t>(mx, (uint32_t)n);
        if (total > 0xFFFFFFFFull) return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "batch exceeds 2^32 packets");
    }
    if (totalPackets) *totalPackets = (uint32_t)total;
    if (maxPacketsPerEvent) *maxPacketsPerEvent = mx;
    return E2SAR_HIP_OK;
}

// Both segmentation entry points: nEvents descriptors, or with devCounts at most that many,
// the count read by the kernel from d_counts[0].
static int segment(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events, bool devCounts, const uint32_t *d_counts,
                   uint32_t nEvents, uint32_t maxPacketsPerEvent, int lbHdrVersion, uint32_t maxPldLen,
                   uint8_t *d_packets, uint32_t stride, uint32_t *d_lens, void *stream)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (nEvents == 0) return E2SAR_HIP_OK;
    if (!d_events || !d_packets || (devCounts && !d_counts)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int rc = check_seg_layout(maxPldLen, stride, d_packets)) return rc;
    return ctx_call(ctx, stream, "seg_kernel launch", [&](hipStream_t s) {
        return launch_segment(d_events, nEvents, maxPacketsPerEvent, lbHdrVersion, maxPldLen, d_packets, stride, d_lens, s,
                              d_counts);
    });
}

int e2sar_hip_segment_batch(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events,
                            uint32_t nEvents, uint32_t maxPacketsPerEvent, int lbHdrVersion,
                            uint32_t maxPldLen, int eventsDwordAligned, uint8_t *d_packets,
                            uint32_t stride, uint32_t *d_lens, void *stream)
{
    (void)eventsDwordAligned;        // a hint only: the kernel checks every event's address itself
    return segment(ctx, d_events, false, nullptr, nEvents, maxPacketsPerEvent, lbHdrVersion, maxPldLen, d_packets, stride,
                   d_lens, stream);
}

int e2sar_hip_segment_batch_dev(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events, const uint32_t *d_counts,
                                uint32_t maxEvents, uint32_t maxPacketsPerEvent, int lbHdrVersion, uint32_t maxPldLen,
                                uint8_t *d_packets, uint32_t stride, uint32_t *d_lens, void *stream)
{
    return segment(ctx, d_events, true, d_counts, maxEvents, maxPacketsPerEvent, lbHdrVersion, maxPldLen, d_packets, stride,
                   d_lens, stream);
}

int e2sar_hip_seg_emit(e2sar_hip_ctx *ctx, const e2sar_hip_seg_source *src, const e2sar_hip_seg_numbering *num,
                       uint32_t maxEvents, int lbHdrVersion, uint32_t maxPldLen, uint8_t *d_packets, uint32_t stride,
                       uint32_t maxPackets, uint32_t *d_lens, e2sar_hip_seg_event *d_events, uint32_t *d_counts,
                       void *stream)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (maxEvents == 0) return E2SAR_HIP_OK;
    if (!src || !num) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL source or numbering");
    if (!src->d_data || !src->d_bytes || !d_packets || !d_events || !d_counts)
        return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if ((src->pitch != 0) == (src->d_offsets != nullptr))
        return fail(E2SAR_HIP_ERR_PARAMETER, "give a pitch (rows) or d_offsets (ragged), not both");
    if (num->flags & ~E2SAR_HIP_SEG_TICKS_AS_EVENTNUM) return fail(E2SAR_HIP_ERR_PARAMETER, "unknown numbering flags");
    if (int rc = check_seg_layout(maxPldLen, stride, d_packets)) return rc;
    if (int rc = check_packets(d_packets, stride, maxPackets)) return rc;
    const uint32_t U = seg_emit_u(src->pitch ? src->pitch : src->maxEventBytes, maxPldLen, stride);
    if (seg_emit_grid(maxEvents, maxPackets, stride, U) > 0x7FFFFFFFull)
        return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "launch too large (units of maxPackets slots + maxEvents)");
    const EmitSrc S{src->d_data, src->dataBytes, src->d_bytes, src->d_offsets, src->d_count, src->pitch};
    const EmitNum N{num->d_eventNums, num->eventNumBase, num->lbTickBase, num->lbTickStep, num->entropyBase, num->dataId,
                    (num->flags & E2SAR_HIP_SEG_TICKS_AS_EVENTNUM) ? 1u : 0u};
    return ctx_call(ctx, stream, "seg_emit launch", [&](hipStream_t s) {
        return launch_seg_emit(S, N, maxEvents, lbHdrVersion, maxPldLen, d_packets, stride, maxPackets, d_lens, d_events,
                               d_counts, U, s);
    });
}

}  // extern "C"

/* ---------------- reassembly straight into a tensor ---------------- */

// What every call of the rows family checks first: the context and the descriptor.  Fills
// the kernels' view of the window.
static int check_rows(const e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, RowsDev &W)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (!w) return fail(E2SAR_HIP_ERR_PARAMETER, "rows descriptor is NULL");
    if (!w->d_out || !w->d_cells || !w->d_base || !w->d_counts) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (!w->dataIds) return fail(E2SAR_HIP_ERR_PARAMETER, "dataIds is NULL");
    if (w->nIds == 0 || w->nIds > E2SAR_HIP_ROWS_MAX_IDS) return fail(E2SAR_HIP_ERR_PARAMETER, "nIds must be 1..64");
    for (uint32_t a = 0; a < w->nIds; a++)
        for (uint32_t b = 0; b < a; b++)
            if (w->dataIds[a] == w->dataIds[b]) return fail(E2SAR_HIP_ERR_PARAMETER, "dataIds must be distinct");
    if (w->nEvents == 0 || (w->nEvents & (w->nEvents - 1u)))
        return fail(E2SAR_HIP_ERR_PARAMETER, "nEvents must be a power of two");
    if (w->pitch == 0 || (w->pitch & 255u)) return fail(E2SAR_HIP_ERR_PARAMETER, "pitch must be a multiple of 256");
    if (int rc = check_pack_out(w->d_out)) return rc;
    if (((uintptr_t)w->d_cells & 15u) || ((uintptr_t)w->d_base & 7u) || ((uintptr_t)w->d_counts & 7u))
        return fail(E2SAR_HIP_ERR_PARAMETER, "cells must be 16-byte aligned, base and counts 8-byte aligned");
    if ((uint64_t)w->nEvents * w->nIds > 0xFFFFFFFFull) return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "more than 2^32 - 1 cells");
    if (w->eventPhase >= std::max(w->eventStep, 1u)) return fail(E2SAR_HIP_ERR_PARAMETER, "eventPhase must be below max(eventStep, 1)");
    W = RowsDev{};
    W.out = w->d_out;
    W.cells = w->d_cells;
    W.base = w->d_base;
    W.counts = w->d_counts;
    W.nIds = w->nIds;
    W.nEvents = w->nEvents;
    W.pitch = w->pitch;
    W.withLB = w->withLBHeader ? 1 : 0;
    std::copy(w->dataIds, w->dataIds + w->nIds, W.ids);
    if (w->eventStep > 1u) {                                          // a lattice; otherwise step, phase and magic stay 0
        const uint64_t S = w->eventStep, top = ~0ull;
        W.step = w->eventStep;
        W.phase = w->eventPhase;
        W.magic = top / S + (top % S == S - 1u ? 1u : 0u);            // floor(2^64 / S): rows_lattice's multiplier
    }
    return E2SAR_HIP_OK;
}

// The seen calls: check_rows, then the bits' descriptor.  Fills the kernels' view of both.
static int check_rows_seen(const e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen, RowsDev &W,
                           RowsSeenDev &Z)
{
    if (int rc = check_rows(ctx, w, W)) return rc;
    if (!seen || !seen->d_seen) return fail(E2SAR_HIP_ERR_PARAMETER, "seen descriptor or d_seen is NULL");
    if (seen->fragBytes == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "fragBytes must be above 0");
    if (seen->maxFrags == 0 || (seen->maxFrags & 127u)) return fail(E2SAR_HIP_ERR_PARAMETER, "maxFrags must be a multiple of 128");
    if ((uintptr_t)seen->d_seen & 15u) return fail(E2SAR_HIP_ERR_PARAMETER, "d_seen must be 16-byte aligned");
    Z = RowsSeenDev{seen->d_seen, rows_div_magic(seen->fragBytes), seen->fragBytes, seen->maxFrags};
    return E2SAR_HIP_OK;
}

extern "C" {

int e2sar_hip_rows_reassemble(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const uint8_t *d_packets, uint32_t stride,
                              const uint32_t *d_lens, const uint32_t *d_count, uint32_t maxPackets, void *stream)
{
    RowsDev W;
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (!w || !d_packets || !d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL descriptor or device buffer");
    if (int rc = check_rows(ctx, w, W)) return rc;
    if (int rc = check_slots(W.withLB != 0, d_packets, stride, maxPackets)) return rc;
    if (maxPackets == 0) return E2SAR_HIP_OK;
    return ctx_call(ctx, stream, "rows reassembly launch", [&](hipStream_t s) -> int {
        if (rows_grid(maxPackets, stride, W.step > 1u) > 0x7FFFFFFFull)
            return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "launch too large (workgroups of maxPackets)");
        const hipError_t e = launch_rows(W, d_packets, stride, d_lens, d_count, maxPackets, s);
        return e == hipSuccess ? E2SAR_HIP_OK : hip_fail(e, "rows reassembly launch");
    });
}

int e2sar_hip_rows_advance(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const uint32_t *d_k, uint32_t kMax, void *stream)
{
    RowsDev W;
    if (int rc = check_rows(ctx, w, W)) return rc;
    return ctx_call(ctx, stream, "rows advance launch", [&](hipStream_t s) { return launch_rows_advance(W, d_k, kMax, s); });
}

int e2sar_hip_rows_clear(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, uint64_t eventBase, void *stream)
{
    RowsDev W;
    if (int rc = check_rows(ctx, w, W)) return rc;
    if (W.step > 1u && eventBase % W.step != W.phase)
        return fail(E2SAR_HIP_ERR_PARAMETER, "eventBase mod eventStep must be eventPhase");
    return ctx_call(ctx, stream, "rows clear launch", [&](hipStream_t s) { return launch_rows_clear(W, eventBase, s); });
}

size_t e2sar_hip_rows_seen_bytes(uint32_t nEvents, uint32_t nIds, uint32_t maxFrags)
{
    return (size_t)nEvents * nIds * (maxFrags / 8u);
}

int e2sar_hip_rows_reassemble_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen,
                                   const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens, const uint32_t *d_count,
                                   uint32_t maxPackets, void *stream)
{
    RowsDev W;
    RowsSeenDev Z;
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (!w || !d_packets || !d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL descriptor or device buffer");
    if (int rc = check_rows_seen(ctx, w, seen, W, Z)) return rc;
    if (int rc = check_slots(W.withLB != 0, d_packets, stride, maxPackets)) return rc;
    if (maxPackets == 0) return E2SAR_HIP_OK;
    return ctx_call(ctx, stream, "rows seen reassembly launch", [&](hipStream_t s) -> int {
        if (rows_seen_grid(maxPackets, stride, W.step > 1u) > 0x7FFFFFFFull)
            return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "launch too large (workgroups of maxPackets)");
        const hipError_t e = launch_rows_seen(W, Z, d_packets, stride, d_lens, d_count, maxPackets, s);
        return e == hipSuccess ? E2SAR_HIP_OK : hip_fail(e, "rows seen reassembly launch");
    });
}

int e2sar_hip_rows_advance_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen, const uint32_t *d_k,
                                uint32_t kMax, void *stream)
{
    RowsDev W;
    RowsSeenDev Z;
    if (int rc = check_rows_seen(ctx, w, seen, W, Z)) return rc;
    if (rows_release_seen_grid(W, Z, kMax) > 0x7FFFFFFFull)
        return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "release launch too large (16-byte words of kMax x nIds cells' bits)");
    return ctx_call(ctx, stream, "rows seen advance launch",
                    [&](hipStream_t s) { return launch_rows_advance_seen(W, Z, d_k, kMax, s); });
}

int e2sar_hip_rows_clear_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen, uint64_t eventBase,
                              void *stream)
{
    RowsDev W;
    RowsSeenDev Z;
    if (int rc = check_rows_seen(ctx, w, seen, W, Z)) return rc;
    if (W.step > 1u && eventBase % W.step != W.phase)
        return fail(E2SAR_HIP_ERR_PARAMETER, "eventBase mod eventStep must be eventPhase");
    return ctx_call(ctx, stream, "rows seen clear launch",
                    [&](hipStream_t s) { return launch_rows_clear_seen(W, Z, eventBase, s); });
}

size_t e2sar_hip_rows_ready_work_bytes(uint32_t nEvents) { return rows_ready_work_bytes(nEvents); }

int e2sar_hip_rows_ready(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_ready_rule *rule, uint32_t *d_ready,
                         e2sar_hip_rows_event *d_events, void *d_work, size_t workBytes, void *stream)
{
    RowsDev W;
    if (int rc = check_rows(ctx, w, W)) return rc;
    if (!rule) return fail(E2SAR_HIP_ERR_PARAMETER, "rule is NULL");
    if (!d_ready || !d_work) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (rule->reserved != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "rule.reserved must be 0");
    if (rule->flags & ~E2SAR_HIP_ROWS_READY_ZERO) return fail(E2SAR_HIP_ERR_PARAMETER, "unknown rule flags");
    const uint64_t all = W.nIds == 64u ? ~0ull : (1ull << W.nIds) - 1ull;
    if (rule->requiredMask & ~all) return fail(E2SAR_HIP_ERR_PARAMETER, "requiredMask names an id at or above nIds");
    if (((uintptr_t)d_work & 255u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "work buffer not 256-byte aligned");
    if (workBytes < rows_ready_work_bytes(W.nEvents)) return fail(E2SAR_HIP_ERR_PARAMETER, "ready work buffer too small");
    if (((uintptr_t)d_ready & 3u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "d_ready not 4-byte aligned");
    if (((uintptr_t)d_events & 7u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "d_events not 8-byte aligned");
    const bool zero = (rule->flags & E2SAR_HIP_ROWS_READY_ZERO) != 0;
    if (zero && rows_zero_grid(W, rule->kMax) > 0x7FFFFFFFull)
        return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "zero launch too large (8-KiB pieces of kMax x nIds cells)");
    // no buffer of the library's, no memset node, no wait: the launches capture as they are
    return ctx_call(ctx, stream, "rows ready launch", [&](hipStream_t s) {
        return launch_rows_ready(W, rule->requiredMask ? rule->requiredMask : all, rule->slack, rule->kMax, zero, d_ready,
                                 d_events, d_work, s);
    });
}

/* ---------------- reassembly ---------------- */

int e2sar_hip_reas_create(e2sar_hip_ctx *ctx, const e2sar_hip_reas_config *cfg, e2sar_hip_reas **out)
{
    if (!ctx || !cfg || !out) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    const uint32_t T = cfg->tableSlots;
    if (T < 64 || (T & (T - 1))) return fail(E2SAR_HIP_ERR_PARAMETER, "tableSlots must be a power of two >= 64");
    if (cfg->queueCapacity == 0 || cfg->lostCapacity == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "zero capacity");
    if (cfg->groupSize > 64) return fail(E2SAR_HIP_ERR_PARAMETER, "groupSize must be 0 (auto) or 1..64");
    HIP_TRY(hipSetDevice(ctx->device));
    // a failure below returns through r's destructor, which releases whatever was built
    auto r = std::make_unique<e2sar_hip_reas>(ctx, *cfg);
    const size_t slotsB = sizeof(ReasSlot) * (size_t)T;
    const size_t ctlB = sizeof(ReasCtl) + (sizeof(ReasShard) + sizeof(ReasOcc)) * kShards;
    const size_t compB = sizeof(e2sar_hip_event_rec) * (size_t)cfg->queueCapacity;
    const size_t lostB = sizeof(e2sar_hip_lost_rec) * (size_t)cfg->lostCapacity;
    const size_t total = slotsB + ctlB + compB + lostB;
    hipError_t e = dev_alloc(r->state, total);
    if (e != hipSuccess) return alloc_fail(e, "hipMalloc(state)");
    // The arenas are plain hipMalloc.  (Round 3: physically contiguous allocations,
    // hipDeviceMallocContiguous, made config 3's scatter 27 % slower at every offset)
    const size_t arenaB = cfg->arenaBytes ? cfg->arenaBytes : 256;
    e = dev_alloc(r->arena[0], arenaB);
    if (e != hipSuccess) return alloc_fail(e, "hipMalloc(arena)");
    // reas_stream_kernel takes a payload's 16-byte phase in its event buffer from the
    // datagram's bufferOffset alone: event buffers are 256-byte aligned in a 256-byte-aligned arena
    if ((reinterpret_cast<uintptr_t>(r->arena[0].get()) & 255u) != 0) return fail(E2SAR_HIP_ERR_MEMORY, "arena not 256-byte aligned");
    auto *base = static_cast<uint8_t *>(r->state.get());
    r->dev.arena = static_cast<uint8_t *>(r->arena[0].get());
    r->dev.slots = reinterpret_cast<ReasSlot *>(base);
    r->dev.ctl = reinterpret_cast<ReasCtl *>(base + slotsB);
    r->dev.shards = reinterpret_cast<ReasShard *>(base + slotsB + sizeof(ReasCtl));
    r->dev.completed = reinterpret_cast<e2sar_hip_event_rec *>(base + slotsB + ctlB);
    r->dev.lost = reinterpret_cast<e2sar_hip_lost_rec *>(base + slotsB + ctlB + compB);
    r->dev.arenaBytes = cfg->arenaBytes;
    r->dev.tableSlots = T;
    r->dev.queueCapacity = cfg->queueCapacity;
    r->dev.lostCapacity = cfg->lostCapacity;
    r->dev.withLB = cfg->withLBHeader ? 1 : 0;
    r->dev.ownWorld = 1;                       // every event is ours until set_owner
    r->dev.ownSelf = 0;
    r->dev.groupSize = cfg->groupSize;
    r->alt = r->dev;
    r->alt.slots = nullptr;          // no alternate table: e2sar_hip_reas_compact refuses
    r->alt.arena = nullptr;
    if (cfg->flags & E2SAR_HIP_REAS_COMPACTABLE) {
        e = dev_alloc(r->altSlots, slotsB);
        if (e == hipSuccess) e = dev_alloc(r->arena[1], arenaB);
        if (e == hipSuccess) e = dev_alloc(r->turnMoves, kTurnMoveBytes * (size_t)T);
        if (e != hipSuccess) return alloc_fail(e, "hipMalloc(alternate arena)");
        r->alt.slots = static_cast<ReasSlot *>(r->altSlots.get());
        r->alt.arena = static_cast<uint8_t *>(r->arena[1].get());
        e = hipMemsetAsync(r->altSlots.get(), 0, slotsB, ctx->stream);
        if (e != hipSuccess) return hip_fail(e, "alternate table init");
    }
    e = hipMemsetAsync(r->state.get(), 0, total, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e, "state init");
    *out = r.release();
    return E2SAR_HIP_OK;
}

void e2sar_hip_reas_destroy(e2sar_hip_reas *r) { delete r; }

uint8_t *e2sar_hip_reas_arena(e2sar_hip_reas *r) { return r ? r->dev.arena : nullptr; }

}  // extern "C"

// Scratch of the reference-order classification for n datagrams on stream s (caller holds r->mu).
static int ro_prepare(e2sar_hip_reas *r, hipStream_t s, uint32_t n)
{
    // the run counters at the front are zero between batches (the kernels reset what they
    // use); a new buffer starts them at zero
    auto &sc = r->scratch[s];
    bool grew = false;
    if (int rc = grow(r, s, sc.ro, ro_scratch_bytes(n, r->dev.tableSlots), &grew)) return rc;
    if (grew) HIP_TRY(hipMemsetAsync(sc.ro.mem.get(), 0, ro_zero_bytes(r->dev.tableSlots), s));
    else if (sc.roDirty) HIP_TRY(launch_fill_bytes(sc.ro.mem.get(), 0, ro_zero_bytes(r->dev.tableSlots), s));  // capture-safe
    sc.roDirty = false;
    return E2SAR_HIP_OK;
}

// launch_ro_classify, remembering a failure part way through its launches (ro_prepare)
static hipError_t ro_classify(e2sar_hip_reas *r, hipStream_t s, const uint8_t *pk, uint32_t stride, const uint32_t *lens,
                              uint32_t n, uint64_t now, void *work)
{
    auto &sc = r->scratch[s];
    const hipError_t e = launch_ro_classify(r->dev, pk, stride, lens, n, now, work, sc.ro.mem.get(), sc.ro.bytes, s);
    if (e != hipSuccess) sc.roDirty = true;
    return e;
}

// The launches of both reassembly entry points on stream s (caller holds r->mu): n
// datagrams, or with d_count min(*d_count, n) of them, the count read by the kernels.
// Everything the host decides, it decides from n: the form, the scatter's loads, the work
// buffer of this stream.
static int reassemble(e2sar_hip_reas *r, hipStream_t s, const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                      const uint32_t *d_count, uint32_t n, uint64_t now_ms)
{
    if (ref_order(r)) {                                   // host count only: the device-count entry point refuses
        // classify in arrival order into the internal work buffer, then the scatter kernel
        auto &sc = r->scratch[s];
        if (int rc = ro_prepare(r, s, n)) return rc;
        if (int rc = grow(r, s, sc.work, work_bytes(n))) return rc;
        void *work = sc.work.mem.get();
        hipError_t e = ro_classify(r, s, d_packets, stride, d_lens, n, now_ms, work);
        if (e == hipSuccess) e = launch_reas_scatter(r->dev, d_packets, stride, n, work, s, cold_loads(r, n, stride));
        if (e != hipSuccess) return hip_fail(e, "reference-order reassembly launch");
        return E2SAR_HIP_OK;
    }
    // A batch whose datagrams cannot still be in the 256 MiB Infinity Cache (more than
    // kFusedMaxBytes of slots) is read back from HBM whatever the caller did before, and
    // there the split form -- classify, then one-round scatter workgroups with streaming
    // loads -- is the faster one: 8 MiB events at MTU 9000, 70 per launch (65,730
    // datagrams, BASELINE config 3): 1116 GiB/s fused vs 1302 split.  Internal work buffer
    // of this stream, grown on first use (outside graph capture).
    if ((uint64_t)n * stride > kFusedMaxBytes) {
        auto &sc = r->scratch[s];
        if (int rc = grow(r, s, sc.work, work_bytes(n))) return rc;
        void *work = sc.work.mem.get();
        hipError_t e = launch_reas_classify(r->dev, d_packets, stride, d_lens, n, now_ms, work, s, d_count);
        if (e == hipSuccess) e = launch_reas_scatter(r->dev, d_packets, stride, n, work, s, true, d_count);
        if (e != hipSuccess)
            return hip_fail(e, d_count ? "reassembly launch (device count, split form)" : "reassembly launch (split form)");
        return E2SAR_HIP_OK;
    }
    const hipError_t e = launch_reassemble(r->dev, d_packets, stride, d_lens, n, now_ms, s, d_count);
    if (e != hipSuccess) return hip_fail(e, d_count ? "reassembly launch (device count)" : "reassembly launch");
    return E2SAR_HIP_OK;
}

extern "C" {

int e2sar_hip_reassemble_batch(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                               const uint32_t *d_lens, uint32_t nPackets, uint64_t now_ms, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (nPackets == 0) return E2SAR_HIP_OK;
    if (!d_packets || !d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int st = check_batch(r, d_packets, stride, nPackets)) return st;
    return reas_launch(r, stream, "reassembly launch", [&](hipStream_t s) {
        return reassemble(r, s, d_packets, stride, d_lens, nullptr, nPackets, now_ms);
    });
}

int e2sar_hip_reassemble_batch_dev(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                                   const uint32_t *d_lens, const uint32_t *d_count, uint32_t maxPackets,
                                   uint64_t now_ms, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    // NULL never means "all" here: a caller with a host count uses e2sar_hip_reassemble_batch
    if (!d_packets || !d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (!d_count) return fail(E2SAR_HIP_ERR_PARAMETER, "d_count is NULL");
    if (int st = check_batch(r, d_packets, stride, maxPackets)) return st;
    if (ref_order(r))
        return fail(E2SAR_HIP_ERR_LOGIC, "a REFERENCE_ORDER reassembler takes its datagram count from the host: its key, "
                                         "place and walk launches are sized by it (use e2sar_hip_reassemble_batch)");
    if (maxPackets == 0) return E2SAR_HIP_OK;
    return reas_launch(r, stream, "reassembly launch (device count)", [&](hipStream_t s) {
        return reassemble(r, s, d_packets, stride, d_lens, d_count, maxPackets, now_ms);
    });
}

#if E2SAR_HIP_EXPERIMENTAL
int e2sar_hip_seg_groups(const e2sar_hip_seg_event *events, uint32_t nEvents, uint32_t maxPacketsPerEvent,
                         uint32_t maxPldLen, uint32_t stride, uint32_t *starts, uint32_t cap, uint32_t *nGroups)
{
    if (!nGroups) return fail(E2SAR_HIP_ERR_PARAMETER, "nGroups is NULL");
    *nGroups = 0;
    if (nEvents && (!events || !starts)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL table");
    // a host-side plan: no packet buffer, and maxPldLen has never been bounded here
    if (int rc = check_seg_layout(maxPldLen, stride, nullptr, false)) return rc;
    *nGroups = seg_groups(events, nEvents, maxPacketsPerEvent, maxPldLen, stride, starts, cap);
    return E2SAR_HIP_OK;
}

int e2sar_hip_reassemble_groups(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                                const uint32_t *d_lens, uint32_t nPackets, const uint32_t *d_starts,
                                uint32_t nGroups, uint64_t now_ms, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (nPackets == 0) return E2SAR_HIP_OK;
    if (nGroups == 0 || !d_starts || ref_order(r) || (uint64_t)nPackets * stride > kFusedMaxBytes)
        return e2sar_hip_reassemble_batch(r, d_packets, stride, d_lens, nPackets, now_ms, stream);
    if (!d_packets || !d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int st = check_batch(r, d_packets, stride, nPackets)) return st;
    if (nGroups > 0x7FFFFFFFu) return fail(E2SAR_HIP_ERR_PARAMETER, "too many groups");
    return reas_launch(r, stream, "reassembly launch (groups)", [&](hipStream_t s) {
        return launch_reassemble_groups(r->dev, d_packets, stride, d_lens, nPackets, d_starts, nGroups, now_ms, s);
    });
}

static int segreas(e2sar_hip_ctx *ctx, const e2sar_hip_segreas_batch *batches, uint32_t nBatches, int lbHdrVersion,
                   uint32_t maxPldLen, uint32_t stride, e2sar_hip_reas *r, uint64_t now_ms, void *stream)
{
    if (!ctx || !r || (!batches && nBatches)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    if (nBatches > kChainMaxBatches) return fail(E2SAR_HIP_ERR_PARAMETER, "more than 8 batches per launch");
    if (int rc = check_seg_layout(maxPldLen, stride, nullptr)) return rc;      // packet buffers: per batch, below
    if (!r->cfg.withLBHeader) return fail(E2SAR_HIP_ERR_PARAMETER, "the chained form emits LB headers: withLBHeader required");
    if (ref_order(r)) return fail(E2SAR_HIP_ERR_PARAMETER, "the chained form is order-insensitive (no REFERENCE_ORDER)");
    ChainBatches cb{};
    uint64_t words = 0;
    for (uint32_t b = 0; b < nBatches; b++) {
        const e2sar_hip_segreas_batch &x = batches[b];
        if (x.nEvents == 0 || x.nPackets == 0) continue;
        if (!x.d_events || !x.d_packets || !x.d_lens) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
        if (int rc = check_packets(x.d_packets, stride, x.nPackets)) return rc;
        for (uint32_t c = 0; c < b; c++)
            if (batches[c].d_packets == x.d_packets && batches[c].nPackets)
                return fail(E2SAR_HIP_ERR_PARAMETER, "batches of one launch need distinct packet buffers");
        ChainBatch &B = cb.b[cb.nb++];
        B.events = x.d_events;
        B.pkts = x.d_packets;
        B.lens = x.d_lens;
        B.nEvents = x.nEvents;
        B.maxPacketsPerEvent = x.maxPacketsPerEvent;
        B.n = x.nPackets;
        B.tiles = reinterpret_cast<uint32_t *>(words);        // offset for now
        words += x.nPackets;
    }
    if (cb.nb == 0) return E2SAR_HIP_OK;
    return reas_launch(r, stream, "segreas_kernel launch", [&](hipStream_t s) -> int {
        auto &sc = r->scratch[s];
        if (int rc = grow(r, s, sc.tiles, 4ull * words)) return rc;
        auto *tiles = static_cast<uint32_t *>(sc.tiles.mem.get());
        for (uint32_t b = 0; b < cb.nb; b++) cb.b[b].tiles = tiles + reinterpret_cast<uintptr_t>(cb.b[b].tiles);
        // the launch's ready counters start at 0: zeroed by a kernel (capture-safe)
        // before every launch, so a group that gave up waiting in an earlier launch (error bit 4)
        // cannot leave a count behind for this one
        hipError_t e = launch_zero_words(tiles, words, s);
        if (e == hipSuccess) e = launch_segreas(cb, lbHdrVersion, maxPldLen, stride, r->dev, now_ms, s);
        if (e != hipSuccess) return hip_fail(e, "segreas_kernel launch");
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_segment_reassemble_batch(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events, uint32_t nEvents,
                                       uint32_t maxPacketsPerEvent, uint32_t nPackets, int lbHdrVersion,
                                       uint32_t maxPldLen, uint8_t *d_packets, uint32_t stride, uint32_t *d_lens,
                                       e2sar_hip_reas *r, uint64_t now_ms, void *stream)
{
    const e2sar_hip_segreas_batch b{d_events, d_packets, d_lens, nEvents, maxPacketsPerEvent, nPackets, 0u};
    return segreas(ctx, &b, 1u, lbHdrVersion, maxPldLen, stride, r, now_ms, stream);
}

int e2sar_hip_segment_reassemble_batches(e2sar_hip_ctx *ctx, const e2sar_hip_segreas_batch *batches,
                                         uint32_t nBatches, int lbHdrVersion, uint32_t maxPldLen, uint32_t stride,
                                         e2sar_hip_reas *r, uint64_t now_ms, void *stream)
{
    return segreas(ctx, batches, nBatches, lbHdrVersion, maxPldLen, stride, r, now_ms, stream);
}

#endif  // E2SAR_HIP_EXPERIMENTAL

int e2sar_hip_relay_plan(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxEvents, size_t maxPldLen,
                         uint64_t lbTick, uint16_t entropyBase, e2sar_hip_seg_event *d_events, uint32_t *d_counts,
                         void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (!d_events || !d_counts) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (maxPldLen == 0 || maxPldLen > 65535u) return fail(E2SAR_HIP_ERR_PARAMETER, "bad maxPldLen");
    return reas_launch(r, stream, "relay_plan launch", [&](hipStream_t s) {
        return launch_relay_plan(r->dev, firstRecord, maxEvents, (uint32_t)maxPldLen, lbTick, entropyBase, d_events,
                                 d_counts, s);
    });
}

int e2sar_hip_reas_collect(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxEvents, uint8_t *d_out,
                           uint64_t outBytes, uint32_t pitch, uint32_t align, e2sar_hip_collect_rec *d_index,
                           uint64_t *d_counts, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (!d_out || !d_index || !d_counts) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (maxEvents == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "maxEvents is 0");
    if (int rc = check_pack_out(d_out)) return rc;
    if (int rc = check_pack_layout(pitch, align)) return rc;
    // no internal buffer, no memset node: the two launches capture as they are
    return reas_launch(r, stream, "collect launch", [&](hipStream_t s) {
        return launch_collect(r->dev, firstRecord, maxEvents, d_out, outBytes, pitch, align, d_index, d_counts, s);
    });
}

int e2sar_hip_reas_collect_next(e2sar_hip_reas *r, uint32_t *d_cursor, uint32_t maxEvents, uint8_t *d_out,
                                uint64_t outBytes, uint32_t pitch, uint32_t align, e2sar_hip_collect_rec *d_index,
                                uint64_t *d_counts, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (!d_cursor) return fail(E2SAR_HIP_ERR_PARAMETER, "cursor is NULL");
    if (!d_out || !d_index || !d_counts) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (maxEvents == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "maxEvents is 0");
    if (int rc = check_pack_out(d_out)) return rc;
    if (int rc = check_pack_layout(pitch, align)) return rc;
    // collect's two launches, with the cursor where firstRecord stood
    return reas_launch(r, stream, "collect_next launch", [&](hipStream_t s) {
        return launch_collect(r->dev, 0u, maxEvents, d_out, outBytes, pitch, align, d_index, d_counts, s, d_cursor);
    });
}

int e2sar_hip_reas_turn(e2sar_hip_reas *r, uint32_t *d_cursor, const e2sar_hip_turn_marks *marks, uint64_t *d_status,
                        void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (!d_cursor || !marks || !d_status) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    if (marks->reserved != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "marks.reserved must be 0");
    // (both set at creation and never changed, so no lock to ask)
    if (!r->alt.slots) return fail(E2SAR_HIP_ERR_LOGIC, "reassembler was not created COMPACTABLE");
    if (ref_order(r))
        return fail(E2SAR_HIP_ERR_LOGIC, "turn is not available in reference-order mode (a slot's carry count would "
                                         "age the key's next item)");
    // no buffer that grows, no memset node, no wait: the four launches capture as they are
    return reas_launch(r, stream, "turn launch", [&](hipStream_t s) {
        return launch_turn(r->dev, r->alt, d_cursor, *marks, d_status, r->turnMoves.get(), s);
    });
}

size_t e2sar_hip_reas_build_work_bytes(uint32_t maxRecords) { return build_work_size(maxRecords); }

int e2sar_hip_reas_build(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxRecords, const uint16_t *dataIds,
                         uint32_t nIds, uint8_t *d_out, uint64_t outBytes, uint32_t pitch, uint32_t align,
                         e2sar_hip_collect_rec *d_members, e2sar_hip_built_rec *d_groups, uint32_t maxGroups,
                         uint64_t *d_counts, void *d_work, size_t workBytes, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (!d_out || !d_members || !d_groups || !d_counts || !d_work) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (maxRecords == 0 || maxRecords > E2SAR_HIP_BUILD_MAX_RECORDS)
        return fail(E2SAR_HIP_ERR_PARAMETER, "maxRecords must be in [1, 4096]");
    if (maxGroups == 0) return fail(E2SAR_HIP_ERR_PARAMETER, "maxGroups is 0");
    if (nIds > E2SAR_HIP_BUILD_MAX_IDS) return fail(E2SAR_HIP_ERR_PARAMETER, "more than 64 dataIds");
    if (nIds && !dataIds) return fail(E2SAR_HIP_ERR_PARAMETER, "dataIds is NULL");
    for (uint32_t a = 0; a < nIds; a++)
        for (uint32_t b = 0; b < a; b++)
            if (dataIds[a] == dataIds[b]) return fail(E2SAR_HIP_ERR_PARAMETER, "a dataId is named twice");
    if (pitch && !nIds) return fail(E2SAR_HIP_ERR_PARAMETER, "cells (pitch > 0) need a dataId list");
    if (int rc = check_pack_layout(pitch, align)) return rc;
    if (int rc = check_pack_out(d_out)) return rc;
    if (((uintptr_t)d_work & 255u) != 0) return fail(E2SAR_HIP_ERR_PARAMETER, "work buffer not 256-byte aligned");
    if (workBytes < build_work_size(maxRecords)) return fail(E2SAR_HIP_ERR_PARAMETER, "build work buffer too small");
    if (outBytes && build_copy_grid(r->dev, maxRecords, nIds, outBytes, pitch, maxGroups) > 0x7FFFFFFFull)
        return fail(E2SAR_HIP_ERR_OUT_OF_RANGE, "copy launch too large (8-KiB pieces of maxGroups x nIds cells)");
    // no internal buffer, no memset node: the two launches capture as they are
    return reas_launch(r, stream, "build launch", [&](hipStream_t s) {
        return launch_build(r->dev, firstRecord, maxRecords, dataIds, nIds, d_out, outBytes, pitch, align, d_members,
                            d_groups, maxGroups, d_counts, d_work, s);
    });
}

size_t e2sar_hip_reas_work_bytes(uint32_t nPackets) { return work_bytes(nPackets); }

int e2sar_hip_reas_classify(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                            const uint32_t *d_lens, uint32_t nPackets, uint64_t now_ms,
                            void *d_work, size_t workBytes, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (nPackets == 0) return E2SAR_HIP_OK;
    if (!d_packets || !d_lens || !d_work) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int st = check_work(d_work, workBytes, nPackets, "work buffer too small")) return st;
    if (int st = check_batch(r, d_packets, stride, nPackets)) return st;
    return reas_launch(r, stream, "classify launch", [&](hipStream_t s) -> int {
        hipError_t e;
        if (ref_order(r)) {
            if (int rc = ro_prepare(r, s, nPackets)) return rc;
            e = ro_classify(r, s, d_packets, stride, d_lens, nPackets, now_ms, d_work);
        } else {
            e = launch_reas_classify(r->dev, d_packets, stride, d_lens, nPackets, now_ms, d_work, s);
        }
        if (e != hipSuccess) return hip_fail(e, "classify launch");
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_reas_scatter(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride, uint32_t nPackets,
                           const void *d_work, size_t workBytes, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (nPackets == 0) return E2SAR_HIP_OK;
    if (!d_packets || !d_work) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int st = check_work(d_work, workBytes, nPackets, "work buffer too small")) return st;
    if (int st = check_batch(r, d_packets, stride, nPackets)) return st;
    return reas_launch(r, stream, "scatter launch", [&](hipStream_t s) {
        return launch_reas_scatter(r->dev, d_packets, stride, nPackets, d_work, s, cold_loads(r, nPackets, stride));
    });
}

int e2sar_hip_reas_scatter_classify(e2sar_hip_reas *r, uint32_t stride, const uint8_t *d_spk, uint32_t sn,
                                    const void *d_swork, size_t sworkBytes, const uint8_t *d_cpk,
                                    const uint32_t *d_clens, uint32_t cn, uint64_t now_ms, void *d_cwork,
                                    size_t cworkBytes, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (sn == 0 && cn == 0) return E2SAR_HIP_OK;
    if (sn) {
        if (!d_spk || !d_swork) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer (scatter batch)");
        if (int st = check_work(d_swork, sworkBytes, sn, "scatter work buffer too small")) return st;
        if (int st = check_batch(r, d_spk, stride, sn)) return st;
    }
    if (cn) {
        if (!d_cpk || !d_clens || !d_cwork) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer (classify batch)");
        if (int st = check_work(d_cwork, cworkBytes, cn, "classify work buffer too small")) return st;
        if (int st = check_batch(r, d_cpk, stride, cn)) return st;
    }
    if (sn && cn && d_swork == d_cwork) return fail(E2SAR_HIP_ERR_PARAMETER, "the two batches need different work buffers");
    return reas_launch(r, stream, "scatter_classify launch", [&](hipStream_t s) -> int {
        hipError_t e;
        if (ref_order(r)) {
            // arrival order needs the classification of b+1 after that of b, not inside the
            // scatter of b: two launches, same results.  (Round 5: the classification of b+1 on
            // a side stream beside the scatter of b measured slower -- the scatter 63 -> 102-113
            // us beside it, DESIGN.md 3 -- so the two run in line.)
            e = launch_reas_scatter(r->dev, d_spk, stride, sn, d_swork, s, cold_loads(r, sn, stride));
            if (e == hipSuccess && cn) {
                if (int rc = ro_prepare(r, s, cn)) return rc;
                e = ro_classify(r, s, d_cpk, stride, d_clens, cn, now_ms, d_cwork);
            }
        } else {
            e = launch_reas_scatter_classify(r->dev, stride, d_spk, sn, d_swork, d_cpk, d_clens, cn, now_ms, d_cwork, s,
                                             cold_loads(r, sn, stride));
        }
        if (e != hipSuccess) return hip_fail(e, "scatter_classify launch");
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_reas_gc(e2sar_hip_reas *r, uint64_t now_ms, uint64_t timeout_ms, void *stream)
{
    return reas_launch(r, stream, "gc launch", [&](hipStream_t s) { return launch_gc(r->dev, now_ms, timeout_ms, s); });
}

// Wait until every kernel launched through this reassembler has finished (caller holds
// r->mu, so no new one starts): an event recorded now on each stream it launched on, not
// the whole device -- other reassemblers, copy streams and unrelated work run on, and a
// capture in progress on another thread is not disturbed.  A stream the caller destroyed
// since (its handle no longer valid) finished its work when it was destroyed.  Once a
// launch of this reassembler has been captured into a graph, its replays can run on any
// stream, so the wait falls back to the device.
static int wait_launches(e2sar_hip_reas *r)
{
    HIP_TRY(hipSetDevice(r->ctx->device));
    if (r->sawCapture) {
        HIP_TRY(hipDeviceSynchronize());
        return E2SAR_HIP_OK;
    }
    if (!r->waitEv) {
        hipEvent_t ev = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        r->waitEv.reset(ev);
    }
    for (auto it = r->streams.begin(); it != r->streams.end();) {
        const hipError_t e = hipEventRecord(r->waitEv.get(), *it);
        if (e == hipErrorInvalidHandle || e == hipErrorContextIsDestroyed || e == hipErrorInvalidResourceHandle) {
            // a stream destroyed without e2sar_hip_reas_forget_stream: its work finished when
            // it was destroyed; its scratch goes with it
            (void)hipGetLastError();
            drop_scratch(r, *it);
            it = r->streams.erase(it);
            continue;
        }
        if (e != hipSuccess) return hip_fail(e, "hipEventRecord");
        HIP_TRY(hipEventSynchronize(r->waitEv.get()));
        ++it;
    }
    // every launch of this reassembler has finished and none was captured, so no kernel and
    // no graph can still hold a buffer that an earlier growth retired: freed
    r->retired.clear();
    return E2SAR_HIP_OK;
}

// The control block with its occupancy counters live: ReasCtl's base plus the ReasOcc shards.
static int read_ctl_occ(e2sar_hip_reas *r, ReasCtl &c)
{
    HIP_TRY(hipMemcpy(&c, r->dev.ctl, sizeof(ReasCtl), hipMemcpyDeviceToHost));
    std::vector<ReasOcc> oc(kShards);
    HIP_TRY(hipMemcpy(oc.data(), r->dev.shards + kShards, sizeof(ReasOcc) * kShards, hipMemcpyDeviceToHost));
    long long used = c.tableUsed;
    for (const auto &x : oc) {
        c.inProgress += x.inProgress;
        used += x.tableUsed;
    }
    c.tableUsed = (uint32_t)used;
    return E2SAR_HIP_OK;
}

// Snapshot of the control block after every launch of this reassembler finished
// (wait_launches), so the read-modify-write of the list counts in poll / lost_poll cannot
// race a kernel's completion atomics.
static int read_ctl(e2sar_hip_reas *r, ReasCtl &c)
{
    if (int rc = wait_launches(r)) return rc;
    HIP_TRY(hipMemcpy(&c, r->dev.ctl, sizeof(ReasCtl), hipMemcpyDeviceToHost));
    return E2SAR_HIP_OK;
}

}  // extern "C"

// Keep records [n, avail) queued by moving them to the front.  hipMemcpy does not allow
// overlapping ranges, so the move goes in chunks of at most n records (each chunk's
// source starts n records above its destination: they never overlap).
template <typename Rec>
static int slide_down(Rec *base, uint32_t n, uint32_t avail)
{
    if (n == 0 || n >= avail) return E2SAR_HIP_OK;
    for (uint32_t d = 0; d < avail - n; d += n) {
        const uint32_t k = std::min(n, avail - n - d);
        HIP_TRY(hipMemcpy(base + d, base + d + n, sizeof(Rec) * k, hipMemcpyDeviceToDevice));
    }
    return E2SAR_HIP_OK;
}

// Hand the first min(cap, queued) records of one of the two device lists to the caller and
// keep the rest queued: the list, its count in ReasCtl and its capacity.
template <typename Rec>
static int poll_list(e2sar_hip_reas *r, Rec *ReasDev::*list, uint32_t ReasCtl::*count, uint32_t ReasDev::*capacity,
                     Rec *out, uint32_t cap, uint32_t *nOut)
{
    if (!r || !nOut || (!out && cap)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    std::lock_guard<std::mutex> lk(r->mu);
    ReasCtl c;
    if (int rc = read_ctl(r, c)) return rc;
    Rec *recs = r->dev.*list;
    const uint32_t avail = std::min(c.*count, r->dev.*capacity);
    const uint32_t n = std::min(avail, cap);
    if (n) HIP_TRY(hipMemcpy(out, recs, sizeof(Rec) * n, hipMemcpyDeviceToHost));
    if (int rc = slide_down(recs, n, avail)) return rc;
    const uint32_t left = avail - n;
    HIP_TRY(hipMemcpy(&(r->dev.ctl->*count), &left, sizeof(uint32_t), hipMemcpyHostToDevice));
    *nOut = n;
    return E2SAR_HIP_OK;
}

extern "C" {

int e2sar_hip_reas_poll(e2sar_hip_reas *r, e2sar_hip_event_rec *out, uint32_t cap, uint32_t *nOut)
{
    return poll_list(r, &ReasDev::completed, &ReasCtl::nCompleted, &ReasDev::queueCapacity, out, cap, nOut);
}

int e2sar_hip_reas_lost_poll(e2sar_hip_reas *r, e2sar_hip_lost_rec *out, uint32_t cap, uint32_t *nOut)
{
    return poll_list(r, &ReasDev::lost, &ReasCtl::nLost, &ReasDev::lostCapacity, out, cap, nOut);
}

int e2sar_hip_reas_get_stats(e2sar_hip_reas *r, e2sar_hip_reas_stats *out)
{
    if (!r || !out) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    std::lock_guard<std::mutex> lk(r->mu);
    ReasCtl c;
    if (int rc = wait_launches(r)) return rc;
    if (int rc = read_ctl_occ(r, c)) return rc;
    // the per-packet counters: summed over the shards
    std::vector<ReasShard> sh(kShards);
    HIP_TRY(hipMemcpy(sh.data(), r->dev.shards, sizeof(ReasShard) * kShards, hipMemcpyDeviceToHost));
    ReasShard t{};
    for (const auto &x : sh) {
        t.totalPackets += x.totalPackets;
        t.totalBytes += x.totalBytes;
        t.badHeaderDiscards += x.badHeaderDiscards;
        t.dataErrCnt += x.dataErrCnt;
        t.eventSuccess += x.eventSuccess;
    }
    out->enqueueLoss = c.enqueueLoss;
    out->reassemblyLoss = c.reassemblyLoss;
    out->eventSuccess = c.eventSuccess + t.eventSuccess;
    out->totalPackets = t.totalPackets;
    out->totalBytes = t.totalBytes;
    out->badHeaderDiscards = t.badHeaderDiscards;
    out->dataErrCnt = t.dataErrCnt;
    out->inProgress = c.inProgress;
    out->completedPending = std::min(c.nCompleted, r->dev.queueCapacity);
    out->lostPending = std::min(c.nLost, r->dev.lostCapacity);
    out->arenaUsed = c.arenaTop;
    out->tableUsed = c.tableUsed;
    out->errorFlags = c.errorFlags;
    out->reserved = 0;
    return E2SAR_HIP_OK;
}

// e2sar_hip_reas_recycle's precondition (caller holds r->mu): without force, the device
// is drained and no event is in progress or unpolled
static int recycle_check(e2sar_hip_reas *r, int force, hipStream_t s)
{
    if (force) return E2SAR_HIP_OK;
    ReasCtl c;
    if (int rc = wait_launches(r)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    if (int rc = read_ctl_occ(r, c)) return rc;
    if (c.inProgress != 0) return fail(E2SAR_HIP_ERR_LOGIC, "events still in progress");
    if (c.nCompleted != 0) return fail(E2SAR_HIP_ERR_LOGIC, "completed events not yet polled");
    return E2SAR_HIP_OK;
}

int e2sar_hip_reas_recycle(e2sar_hip_reas *r, int force, void *stream)
{
    return reas_launch(r, stream, "recycle launch", [&](hipStream_t s) -> int {
        if (int rc = recycle_check(r, force, s)) return rc;
        const hipError_t e = launch_recycle(r->dev, force != 0, s);
        if (e != hipSuccess) return hip_fail(e, "recycle launch");
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_segment_batch_recycle(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events, uint32_t nEvents,
                                    uint32_t maxPacketsPerEvent, int lbHdrVersion, uint32_t maxPldLen,
                                    int eventsDwordAligned, uint8_t *d_packets, uint32_t stride, uint32_t *d_lens,
                                    e2sar_hip_reas *r, int force, void *stream)
{
    if (!ctx) return fail(E2SAR_HIP_ERR_PARAMETER, "ctx is NULL");
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (r->ctx->device != ctx->device) return fail(E2SAR_HIP_ERR_PARAMETER, "reassembler on another device");
    if (nEvents && (!d_events || !d_packets)) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (int rc = check_seg_layout(maxPldLen, stride, d_packets)) return rc;
    (void)eventsDwordAligned;
    // unlike its siblings, on the segmenter context's device and default stream, not r's
    return reas_launch(r, stream, "seg_kernel + recycle launch", [&](hipStream_t s) -> int {
        if (int rc = recycle_check(r, force, s)) return rc;
        const hipError_t e = launch_segment(d_events, nEvents, maxPacketsPerEvent, lbHdrVersion, maxPldLen, d_packets,
                                            stride, d_lens, s, nullptr, &r->dev, force != 0);
        if (e != hipSuccess) return hip_fail(e, "seg_kernel + recycle launch");
        return E2SAR_HIP_OK;
    }, ctx);
}

int e2sar_hip_reas_compact(e2sar_hip_reas *r, void *stream)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    // (set at creation: whether the alternate table exists never changes, so no lock to ask)
    if (!r->alt.slots) return fail(E2SAR_HIP_ERR_LOGIC, "reassembler was not created COMPACTABLE");
    return reas_launch(r, stream, "compact launch", [&](hipStream_t s) -> int {
        ReasCtl c;
        if (int rc = wait_launches(r)) return rc;
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipMemcpy(&c, r->dev.ctl, sizeof(ReasCtl), hipMemcpyDeviceToHost));
        if (c.nCompleted != 0) return fail(E2SAR_HIP_ERR_LOGIC, "completed events not yet polled");
        const hipError_t e = launch_compact(r->dev, r->alt, s);
        if (e != hipSuccess) return hip_fail(e, "compact launch");
        std::swap(r->dev.slots, r->alt.slots);
        std::swap(r->dev.arena, r->alt.arena);
        return E2SAR_HIP_OK;
    });
}

int e2sar_hip_reas_reset_stats(e2sar_hip_reas *r, void *stream)
{
    return reas_launch(r, stream, "reset_stats launch", [&](hipStream_t s) -> int {
        // the event counters (eventSuccess .. reassemblyLoss), the per-packet shards and the
        // error flags; the completed / lost records not yet polled stay queued (resetting
        // statistics in the reference discards no queued event), and so does inProgress, which
        // counts live table entries, not history
        auto *ctl = reinterpret_cast<uint8_t *>(r->dev.ctl);
        // kernels, not memset nodes: this call may be captured into a HIP graph
        HIP_TRY(launch_zero_words(ctl + offsetof(ReasCtl, eventSuccess),
                                  (offsetof(ReasCtl, inProgress) - offsetof(ReasCtl, eventSuccess)) / 4, s));
        HIP_TRY(launch_zero_words(r->dev.shards, sizeof(ReasShard) * kShards / 4, s));
        HIP_TRY(launch_zero_words(ctl + offsetof(ReasCtl, errorFlags), 1, s));
        return E2SAR_HIP_OK;
    });
}

size_t e2sar_hip_route_workspace_bytes(uint32_t nPackets, uint32_t world)
{
    return route_workspace_bytes(nPackets, world);
}

}  // extern "C"

static int route(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                 uint32_t nPackets, int withLBHeader, uint32_t world, uint32_t self, int excludeSelf,
                 uint8_t *d_sendPackets, uint32_t *d_sendLens, uint32_t *d_counts, void *d_workspace,
                 size_t workspaceBytes, void *stream)
{
    if (int rc = check_route(ctx, world, self, stride)) return rc;
    if (nPackets && (!d_packets || !d_lens || !d_sendPackets || !d_sendLens || !d_counts || !d_workspace))
        return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    if (workspaceBytes < route_workspace_bytes(nPackets, world)) return fail(E2SAR_HIP_ERR_PARAMETER, "workspace too small");
    return ctx_call(ctx, stream, "route launch", [&](hipStream_t s) {
        return launch_route(d_packets, stride, d_lens, nPackets, withLBHeader, world, self, excludeSelf, d_sendPackets,
                            d_sendLens, d_counts, d_workspace, s);
    });
}

extern "C" {

int e2sar_hip_route_batch(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                          uint32_t nPackets, int withLBHeader, uint32_t world, uint32_t self, uint8_t *d_sendPackets,
                          uint32_t *d_sendLens, uint32_t *d_counts, void *d_workspace, size_t workspaceBytes,
                          void *stream)
{
    return route(ctx, d_packets, stride, d_lens, nPackets, withLBHeader, world, self, 0, d_sendPackets, d_sendLens,
                 d_counts, d_workspace, workspaceBytes, stream);
}

int e2sar_hip_route_foreign(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                            uint32_t nPackets, int withLBHeader, uint32_t world, uint32_t self,
                            uint8_t *d_sendPackets, uint32_t *d_sendLens, uint32_t *d_counts, void *d_workspace,
                            size_t workspaceBytes, void *stream)
{
    return route(ctx, d_packets, stride, d_lens, nPackets, withLBHeader, world, self, 1, d_sendPackets, d_sendLens,
                 d_counts, d_workspace, workspaceBytes, stream);
}

int e2sar_hip_route_append(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                           uint32_t nPackets, int withLBHeader, uint32_t world, uint32_t self, int foreignOnly,
                           uint8_t *d_sendPackets, uint32_t *d_sendLens, uint32_t capPerRank, uint32_t *d_running,
                           void *d_workspace, size_t workspaceBytes, void *stream)
{
    if (int rc = check_route(ctx, world, self, stride)) return rc;
    if (capPerRank == 0 || (uint64_t)capPerRank * world > 0xFFFFFFFFull)
        return fail(E2SAR_HIP_ERR_PARAMETER, "capPerRank must be > 0 and capPerRank * world < 2^32");
    if (!d_running) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL running counters");
    if (nPackets && (!d_packets || !d_lens || !d_sendPackets || !d_sendLens))
        return fail(E2SAR_HIP_ERR_PARAMETER, "NULL device buffer");
    (void)d_workspace;
    (void)workspaceBytes;                  // one launch, no workspace (kept in the signature for callers)
    return ctx_call(ctx, stream, "route launch", [&](hipStream_t s) {
        return launch_route_append(d_packets, stride, d_lens, nPackets, withLBHeader, world, self, foreignOnly ? 1 : 0,
                                   d_sendPackets, d_sendLens, capPerRank, d_running, s);
    });
}

int e2sar_hip_reas_set_owner(e2sar_hip_reas *r, uint32_t world, uint32_t self)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    if (int rc = check_world(world, self)) return rc;
    std::lock_guard<std::mutex> lk(r->mu);
    r->dev.ownWorld = r->alt.ownWorld = world;
    r->dev.ownSelf = r->alt.ownSelf = self;
    return E2SAR_HIP_OK;
}

int e2sar_hip_reas_forget_stream(e2sar_hip_reas *r, void *stream)
{
    if (!r || !stream) return fail(E2SAR_HIP_ERR_PARAMETER, "NULL argument");
    std::lock_guard<std::mutex> lk(r->mu);
    HIP_TRY(hipSetDevice(r->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HIP_TRY(hipStreamSynchronize(s));
    r->streams.erase(s);
    drop_scratch(r, s);
    return E2SAR_HIP_OK;
}

int e2sar_hip_reas_set_cold(e2sar_hip_reas *r, int cold)
{
    if (!r) return fail(E2SAR_HIP_ERR_PARAMETER, "reas is NULL");
    std::lock_guard<std::mutex> lk(r->mu);
    if (cold) r->cfg.flags |= E2SAR_HIP_REAS_COLD_DATAGRAMS;
    else r->cfg.flags &= ~E2SAR_HIP_REAS_COLD_DATAGRAMS;
    return E2SAR_HIP_OK;
}

}  // extern "C"
