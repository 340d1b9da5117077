/*
 * e2sar_hip.h -- C ABI of the MI355X (gfx950) SAR data path.
 *
 * This is the drop-in boundary for the reference's segmentation / reassembly hot path
 * (JeffersonLab/E2SAR v0.3.2).  Plain C: pointers, sizes, integer status codes; no HIP,
 * torch or C++ types cross it.  Device pointers are passed as ordinary pointers that
 * were allocated on the context's device (hipMalloc, torch, or e2sar_hip_device_alloc).
 *
 * Each entry point names the reference interface it replaces (file:line).
 *
 * Status codes: 0 = success, negative = -(E2SARErrorc) from include/e2sarError.hpp:23-39
 * (e.g. -3 ParameterError, -5 OutOfRange, -7 NotFound, -10 MemoryError, -11 LogicError,
 * -12 SystemError for a HIP runtime failure, -13 DataError).  No C++ exception crosses
 * this boundary (the reference methods are noexcept, e2sarDPSegmenter.hpp:458-483).
 */
#ifndef E2SAR_HIP_H
#define E2SAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define E2SAR_HIP_ABI_VERSION 1

enum {
    E2SAR_HIP_OK = 0,
    E2SAR_HIP_ERR_PARAMETER = -3,   /* E2SARErrorc::ParameterError */
    E2SAR_HIP_ERR_OUT_OF_RANGE = -5,/* E2SARErrorc::OutOfRange */
    E2SAR_HIP_ERR_NOT_FOUND = -7,   /* E2SARErrorc::NotFound */
    E2SAR_HIP_ERR_MEMORY = -10,     /* E2SARErrorc::MemoryError */
    E2SAR_HIP_ERR_LOGIC = -11,      /* E2SARErrorc::LogicError */
    E2SAR_HIP_ERR_SYSTEM = -12,     /* E2SARErrorc::SystemError (HIP runtime failure) */
    E2SAR_HIP_ERR_DATA = -13        /* E2SARErrorc::DataError */
};

/* LB+RE header geometry on the wire (e2sarHeaders.hpp:302-315): 16-byte LB + 20-byte RE */
#define E2SAR_HIP_LB_HDR_LEN 16
#define E2SAR_HIP_RE_HDR_LEN 20
#define E2SAR_HIP_LBRE_HDR_LEN 36

/* ------------------------------------------------------------------ */
/* library / context                                                   */

int e2sar_hip_abi_version(void);
/* Human-readable message for the last failing call on this thread (E2SARErrorInfo::msg). */
const char *e2sar_hip_last_error(void);

typedef struct e2sar_hip_ctx e2sar_hip_ctx;
/* Bind a device and a stream.  `stream` is the hipStream_t every call of this context
 * runs on when the call's own `stream` argument is NULL; NULL here means the device's
 * default stream.  Replaces the per-Segmenter/Reassembler thread state
 * (e2sarDPSegmenter.hpp:213-260, e2sarDPReassembler.hpp:206-240): one context per
 * sending/receiving thread gives the same concurrency without shared mutable state. */
int e2sar_hip_ctx_create(int device, void *stream, e2sar_hip_ctx **out);
/* A non-blocking stream for callers without a HIP toolchain. */
int e2sar_hip_stream_create(int device, void **out);
int e2sar_hip_stream_destroy(void *stream);
/* Every reassembler created on a context holds a reference to it: a context and its
 * reassemblers may be destroyed in any order (the memory goes with the last of them). */
void e2sar_hip_ctx_destroy(e2sar_hip_ctx *ctx);
void *e2sar_hip_ctx_stream(e2sar_hip_ctx *ctx);
int e2sar_hip_ctx_device(e2sar_hip_ctx *ctx);
int e2sar_hip_ctx_sync(e2sar_hip_ctx *ctx);

/* memory plumbing so callers without a HIP toolchain (cgo/ctypes/C++) can drive the path */
int e2sar_hip_device_alloc(e2sar_hip_ctx *ctx, size_t bytes, void **out);
int e2sar_hip_device_free(e2sar_hip_ctx *ctx, void *p);
int e2sar_hip_host_alloc(size_t bytes, void **out);           /* pinned host memory */
int e2sar_hip_host_free(void *p);
int e2sar_hip_memcpy_h2d(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes);
int e2sar_hip_memcpy_d2h(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes);
/* fill `bytes` device bytes with (uint8_t)value on the context stream: a kernel, not
 * hipMemsetAsync, so the call may be captured into a HIP graph (captured memset nodes write
 * garbage from the second replay on with this ROCm) */
int e2sar_hip_memset_d(e2sar_hip_ctx *ctx, void *dst, int value, size_t bytes);
/* e2sar_hip_memset_d on `stream` (NULL = context stream): a fill kernel, capture-safe */
int e2sar_hip_memset_async(e2sar_hip_ctx *ctx, void *dst, int value, size_t bytes, void *stream);
/* asynchronous copy on `stream` (NULL = context stream); kind 0 = H2D, 1 = D2H, 2 = D2D */
int e2sar_hip_memcpy_async(e2sar_hip_ctx *ctx, void *dst, const void *src, size_t bytes, int kind,
                           void *stream);
int e2sar_hip_stream_sync(e2sar_hip_ctx *ctx, void *stream);

/* stream ordering for callers without a HIP toolchain (the C++ facade pipelines its
 * host->device copies beside the reassembly kernels with these): an event records the
 * point a stream has reached; another stream can wait for it, the host can query or wait. */
int e2sar_hip_event_create(e2sar_hip_ctx *ctx, void **out);
int e2sar_hip_event_destroy(void *event);
int e2sar_hip_event_record(e2sar_hip_ctx *ctx, void *event, void *stream);   /* NULL stream = context stream */
int e2sar_hip_stream_wait_event(e2sar_hip_ctx *ctx, void *stream, void *event);
int e2sar_hip_event_query(void *event);        /* 1 = reached, 0 = not yet, < 0 = error */
int e2sar_hip_event_sync(void *event);

/* Gather copy: n spans {src, dst, bytes}, device or pinned host memory on either side
 * (pinned memory from e2sar_hip_host_alloc is device-accessible at the same address), in
 * one kernel launch per 64 spans on `stream`.  This is how completed events leave the
 * device arena in one batch instead of one memcpy per event. */
typedef struct e2sar_hip_copy_span {
    const void *src;
    void *dst;
    uint64_t bytes;
} e2sar_hip_copy_span;
int e2sar_hip_copy_spans(e2sar_hip_ctx *ctx, const e2sar_hip_copy_span *spans, uint32_t n, void *stream);

/* ------------------------------------------------------------------ */
/* geometry (e2sarHeaders.hpp:415-421, e2sarDPSegmenter.hpp:241, e2sarDPSegmenter.cpp:670) */

size_t e2sar_hip_total_hdr_len(int useIPv6);                 /* 64 (v4) / 84 (v6) */
size_t e2sar_hip_max_pld_len(uint32_t mtu, int useIPv6);     /* mtu - total_hdr_len; 0 if mtu too small */
size_t e2sar_hip_num_packets(size_t bytes, size_t maxPldLen);/* ceil(bytes / maxPldLen) */
/* device packet slot: 36 + maxPldLen rounded up to 16 bytes */
uint32_t e2sar_hip_packet_stride(size_t maxPldLen);

/* ------------------------------------------------------------------ */
/* segmentation: replaces SendThreadState::_send's fragment loop        */
/* (e2sarDPSegmenter.cpp:660-871) for a batch of events                 */

/* One event: the arguments of _send (cpp:660-662) after the host has applied the
 * event-numbering rule (cpp:901-917 / 920-948), the dataId default (cpp:938), entropy
 * "0 => random" (cpp:727-728), the LB tick (cpp:707-719) and ticksAsREEventNum
 * (cpp:723-724).  40 bytes, 8-byte aligned. */
typedef struct e2sar_hip_seg_event {
    const uint8_t *data;   /* device address of the event bytes */
    uint64_t eventNum;     /* RE eventNum */
    uint64_t lbTick;       /* LB eventNum (v2) / tick (v3) */
    uint32_t bytes;        /* event length; REHdr bufferLength is u32 (e2sarHeaders.hpp:26) */
    uint32_t pktBase;      /* index of the event's first packet in the batch (set by seg_plan) */
    uint16_t dataId;
    uint16_t entropy;
    uint32_t reserved;
} e2sar_hip_seg_event;

/* Host-side plan over a host copy of the event table: fills pktBase (exclusive prefix
 * of ceil(bytes/maxPldLen)) and writes the batch's packet count and the largest per-event
 * packet count to *totalPackets and *maxPacketsPerEvent (either may be NULL).  Returns a
 * status: 0, or E2SAR_HIP_ERR_PARAMETER (NULL table, maxPldLen 0) / OUT_OF_RANGE (more
 * than 2^32 - 1 packets). */
int e2sar_hip_seg_plan(e2sar_hip_seg_event *events, uint32_t nEvents, size_t maxPldLen,
                       uint32_t *totalPackets, uint32_t *maxPacketsPerEvent);

/* Segment nEvents events (descriptor table `d_events` already on the device) into
 * datagrams [16-byte LB][20-byte RE][payload] at d_packets + p*stride, p = pktBase+k.
 * d_lens[p] (optional) receives the datagram length 36 + payload.  Padding: the bytes from
 * the datagram's end to the end of its last 16-byte chunk are zero, and the rest of the slot
 * (stride: any multiple of 16 that holds 36 + maxPldLen) is not written.  lbHdrVersion 3
 * selects LBHdrV3, any other value LBHdrV2 (e2sarHeaders.hpp:287-297).
 * maxPacketsPerEvent: an upper bound (from seg_plan).  eventsDwordAligned is a hint kept
 * for ABI compatibility: the kernel takes its 16-byte dword-aligned fast path for every
 * event whose address and maxPldLen are multiples of 4 and a byte path for the others,
 * checking each event itself.  Asynchronous on `stream` (NULL = the context stream). */
int e2sar_hip_segment_batch(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events,
                            uint32_t nEvents, uint32_t maxPacketsPerEvent,
                            int lbHdrVersion, uint32_t maxPldLen, int eventsDwordAligned,
                            uint8_t *d_packets, uint32_t stride, uint32_t *d_lens,
                            void *stream);

/* ------------------------------------------------------------------ */
/* reassembly: replaces the RecvThreadState per-packet body             */
/* (e2sarDPReassembler.cpp:310-428), eventsInProgress (hpp:224-233),    */
/* the event queue (hpp:126-161) and the GC pass (cpp:236-291)          */

typedef struct e2sar_hip_reas e2sar_hip_reas;

typedef struct e2sar_hip_reas_config {
    int withLBHeader;          /* ReassemblerFlags::withLBHeader (hpp:436) */
    uint32_t tableSlots;       /* in-progress event table slots (power of two, >= 64) */
    uint32_t queueCapacity;    /* completed-event records held until polled (QSIZE, hpp:126) */
    uint32_t lostCapacity;     /* lost-event records held until polled */
    uint64_t arenaBytes;       /* device arena that receives reassembled event bytes */
    uint32_t flags;            /* E2SAR_HIP_REAS_* */
    uint32_t groupSize;        /* datagrams per workgroup of the fused reassembly kernel (1..64);
                                  0 = automatic: a 9K-chunk budget balanced to whole residency
                                  waves of the chip (the measured best) */
} e2sar_hip_reas_config;

/* Allocate a second table + arena so e2sar_hip_reas_compact() can move in-progress
 * events out of a full arena (streaming use: events that straddle batches). */
#define E2SAR_HIP_REAS_COMPACTABLE 1u
/* Reassemble with the reference receive body's arrival-order rules, whatever the order:
 * a fragment with bufferOffset 0 always starts a new item, dropping an item in progress
 * under the same (eventNum, dataId) without a lost record (e2sarDPReassembler.cpp:361-369);
 * a fragment whose key has no item starts one, also after its event completed
 * (cpp:376-384); completion is tested after every fragment (cpp:403), so duplicates
 * before the last fragment overshoot curBytes.  Arrival order = batch order, then datagram
 * order in the batch.  Without the flag the device path is order-insensitive: every
 * fragment joins its event and completion is tested per run of a launch (identical results
 * whenever offset 0 arrives first and there are no duplicates).  The mode
 * adds a key pass and a per-key walk per batch and device scratch (about 56 bytes per
 * datagram of the largest batch, 48 more in reassemble_batch for its work records, and 524
 * bytes per table slot) that grows on demand (per stream; it cannot
 * grow inside a graph capture -- such a launch fails with LOGIC -- so capture only after a
 * first batch of the largest size has run on the capturing stream). */
#define E2SAR_HIP_REAS_REFERENCE_ORDER 2u
/* The datagram batches of this reassembler were written long before they are reassembled
 * (not in the Infinity Cache, e.g. received into HBM well ahead): the split, pipelined and
 * reference-order forms read them with streaming (non-temporal) loads.  Without the flag
 * they use cache-allocating loads (a batch just written -- by the segmenter, a copy, the NIC
 * -- is read from cache), except for batches above 320 MiB of slots, which cannot be. */
#define E2SAR_HIP_REAS_COLD_DATAGRAMS 4u

/* Reassembled event handed to the caller (getEvent's out-params, cpp:626-641).
 * The bytes live at e2sar_hip_reas_arena() + arenaOffset until the arena is recycled. */
typedef struct e2sar_hip_event_rec {
    uint64_t eventNum;
    uint64_t arenaOffset;
    uint32_t bytes;
    uint16_t dataId;
    uint16_t flags;
    uint32_t numFragments;
    uint32_t reserved;
} e2sar_hip_event_rec;

/* get_LostEvent's tuple (hpp:593-604) + which loss it was. */
typedef struct e2sar_hip_lost_rec {
    uint64_t eventNum;
    uint64_t numFragments;
    uint16_t dataId;
    uint16_t enqueueLoss;      /* 1 = lost on enqueue (queue/arena full), 0 = reassembly (GC) */
    uint32_t reserved;
} e2sar_hip_lost_rec;

/* Reassembler::ReportedStats (hpp:383-400) plus device-path diagnostics. */
typedef struct e2sar_hip_reas_stats {
    uint64_t enqueueLoss;
    uint64_t reassemblyLoss;
    uint64_t eventSuccess;
    uint64_t totalPackets;
    uint64_t totalBytes;
    uint64_t badHeaderDiscards;
    uint64_t dataErrCnt;
    int64_t inProgress;
    uint64_t completedPending;   /* records waiting in the completion list */
    uint64_t lostPending;
    uint64_t arenaUsed;
    uint64_t tableUsed;          /* slots ever claimed since the last recycle */
    uint32_t errorFlags;         /* bit0 table full, bit1 arena full, bit2 probe timeout,
                                    bit3 scatter record outside the arena (bad work buffer),
                                    bit4 chained form: a group's datagrams never all written
                                    (wait timed out), bit5 chained form: counter over-count */
    uint32_t reserved;
} e2sar_hip_reas_stats;

int e2sar_hip_reas_create(e2sar_hip_ctx *ctx, const e2sar_hip_reas_config *cfg,
                          e2sar_hip_reas **out);
void e2sar_hip_reas_destroy(e2sar_hip_reas *r);
/* device base of the event arena */
uint8_t *e2sar_hip_reas_arena(e2sar_hip_reas *r);

/* Parse, validate, look up / create and scatter nPackets datagrams held at
 * d_packets + p*stride with lengths d_lens[p] (the full datagram length as recvfrom
 * returns it, cpp:321).  now_ms stamps firstSegment for new events (hpp:97).
 * One fused launch for batches of up to 320 MiB of slots; above that (a batch that cannot
 * sit in the Infinity Cache) classify + scatter launches through an internal work buffer.
 * Internal buffers (this form, reference order) are kept per stream, so batches may be launched on several streams at once; they grow on first
 * use for a size, never inside a graph capture (LOGIC error: run one batch of the largest
 * size on the stream first).  Once a launch has been captured, an outgrown buffer stays
 * allocated until destroy, so a graph captured earlier keeps valid addresses; before that it
 * is freed by the next call that waits for this reassembler's launches (poll, lost_poll,
 * get_stats, compact, recycle without force).
 * Asynchronous on `stream` (NULL = the context stream). */
int e2sar_hip_reassemble_batch(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                               const uint32_t *d_lens, uint32_t nPackets, uint64_t now_ms,
                               void *stream);

/* e2sar_hip_reassemble_batch for a batch whose datagram count lives on the device: the
 * datagrams [0, n), n = min(*d_count, maxPackets), are reassembled, where *d_count is a
 * device uint32 the kernels read when they run -- d_counts + 1 of e2sar_hip_seg_emit or of
 * e2sar_hip_relay_plan, for instance.  The host never reads it, so a device-side
 * segmentation feeds a reassembler without a wait, and the chain producer -> emit ->
 * reassemble -> collect / build may be captured as one graph and replayed with another
 * count each time.  Replaces the same per-packet body (e2sarDPReassembler.cpp:310-428).
 *   No byte of a slot at or past n and no d_lens entry at or past n is read.  n == 0 changes
 * nothing in the reassembler: no counter, no table slot, no arena byte.  Events, bytes,
 * numFragments, every statistic and every lost record are those of
 * e2sar_hip_reassemble_batch(..., n, ...) on the same datagrams, whenever that result does
 * not depend on how a launch is cut into groups (offset 0 first, no duplicates: DESIGN.md
 * 5.3) -- the groups here are cut for maxPackets, not for n.
 *   All launch geometry comes from maxPackets: the group size (unless cfg.groupSize fixes
 * it), the grid, the fused form or -- above 320 MiB of slots -- the split form, streaming
 * loads for a batch that large, and the size and layout of the split form's internal work
 * buffer (per stream, grown on first use, never inside a graph capture: LOGIC, as above).
 * One kernel launch, two in the split form; after a stream's first use no allocation, no
 * memset node, no wait: the call may be captured into a HIP graph.  A workgroup past n
 * costs the load of one word.  set_owner, set_cold, the stream default and the waits of
 * poll / lost_poll / get_stats are those of e2sar_hip_reassemble_batch.
 *   Status: PARAMETER for a NULL r, d_packets, d_lens or d_count (NULL does not mean "all":
 * a caller with a host count uses e2sar_hip_reassemble_batch); then the stride and batch
 * checks of e2sar_hip_reassemble_batch, applied to maxPackets; LOGIC for a reassembler
 * created with E2SAR_HIP_REAS_REFERENCE_ORDER -- that mode's key, place and walk launches
 * and its scratch layout are sized by the datagram count, and giving them a device count
 * means editing those kernels: not yet done.  maxPackets == 0 succeeds and launches
 * nothing.  A failing call launches nothing.  Asynchronous on `stream` (NULL = the context
 * stream). */
int e2sar_hip_reassemble_batch_dev(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                                   const uint32_t *d_lens, const uint32_t *d_count,
                                   uint32_t maxPackets, uint64_t now_ms, void *stream);

/* The same work as e2sar_hip_reassemble_batch split in two phases so a caller can
 * pipeline batches: classify (headers only: validate, look up / create, count) writes
 * per-datagram destinations into d_work; scatter moves the payload bytes and publishes
 * the events the batch completed.  Scatter a batch after its classify (same packets,
 * stride, nPackets and work buffer, ordered on one stream or by an event); the work
 * buffer is reusable once that scatter has run.  Batches are classified in arrival order.
 * d_work: device memory, 256-byte aligned, e2sar_hip_reas_work_bytes(nPackets) bytes;
 * no initialisation needed.  Asynchronous.  Replaces the same per-packet body
 * (e2sarDPReassembler.cpp:335-427) as e2sar_hip_reassemble_batch. */
size_t e2sar_hip_reas_work_bytes(uint32_t nPackets);
int e2sar_hip_reas_classify(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                            const uint32_t *d_lens, uint32_t nPackets, uint64_t now_ms,
                            void *d_work, size_t workBytes, void *stream);
int e2sar_hip_reas_scatter(e2sar_hip_reas *r, const uint8_t *d_packets, uint32_t stride,
                           uint32_t nPackets, const void *d_work, size_t workBytes, void *stream);
/* Pipelined step, one launch: scatter the classified batch b (d_spk, sn, d_swork) while
 * other workgroups of the same grid classify batch b+1 (d_cpk, d_clens, cn, d_cwork).
 * The two batches use different packet and work buffers.  A stream of batches runs as
 * classify(0), scatter_classify(0, 1), ..., scatter_classify(k-1, k), scatter(k). */
int e2sar_hip_reas_scatter_classify(e2sar_hip_reas *r, uint32_t stride,
                                    const uint8_t *d_spk, uint32_t sn, const void *d_swork,
                                    size_t sworkBytes, const uint8_t *d_cpk,
                                    const uint32_t *d_clens, uint32_t cn, uint64_t now_ms,
                                    void *d_cwork, size_t cworkBytes, void *stream);

/* GC pass: events whose first fragment is older than timeout_ms become lost
 * (reassemblyLoss, cpp:252-274).  Asynchronous. */
int e2sar_hip_reas_gc(e2sar_hip_reas *r, uint64_t now_ms, uint64_t timeout_ms, void *stream);

/* Drain completed events.  Waits, under the reassembler's lock, for every kernel launched
 * through this reassembler (an event recorded after each launch on each stream used; other
 * streams and reassemblers are not waited for), so none runs while the list is drained.
 * Once a launch of this reassembler has been captured into a HIP graph, replays may run on
 * any stream and the wait covers the whole device.  Records are returned in completion
 * order of the device; *nOut <= cap.  Records beyond cap stay queued. */
int e2sar_hip_reas_poll(e2sar_hip_reas *r, e2sar_hip_event_rec *out, uint32_t cap,
                        uint32_t *nOut);
/* Drain lost-event records (waits for this reassembler's launches, as reas_poll). */
int e2sar_hip_reas_lost_poll(e2sar_hip_reas *r, e2sar_hip_lost_rec *out, uint32_t cap,
                             uint32_t *nOut);
/* Stats snapshot (waits for this reassembler's launches, as reas_poll). */
int e2sar_hip_reas_get_stats(e2sar_hip_reas *r, e2sar_hip_reas_stats *out);
/* Recycle the arena and the event table.  Only legal when no event is in progress
 * and every completed record has been polled (else E2SAR_HIP_ERR_LOGIC); the caller
 * promises it no longer reads event bytes from the arena.  `force` drops in-progress
 * events without logging them.  It also discards completed records not yet polled (the
 * bench's step relies on that); lost records not yet polled and the statistics stay.
 * Asynchronous. */
int e2sar_hip_reas_recycle(e2sar_hip_reas *r, int force, void *stream);
/* e2sar_hip_segment_batch and e2sar_hip_reas_recycle(r, force) in ONE launch: extra
 * workgroups at the end of the segmentation grid reset r's table and arena (no seg block
 * touches them).  Same preconditions as the two calls; r's earlier launches on `stream`
 * finish before it starts, and its next reassembly starts after it.  What it saves is one
 * launch and its boundary per step (the bench's step: recycle, then segment -> reassemble
 * per batch).  Replaces nothing in the reference (whose events are new[] buffers); see
 * e2sar_hip_reas_recycle. */
int e2sar_hip_segment_batch_recycle(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events, uint32_t nEvents,
                                    uint32_t maxPacketsPerEvent, int lbHdrVersion, uint32_t maxPldLen,
                                    int eventsDwordAligned, uint8_t *d_packets, uint32_t stride, uint32_t *d_lens,
                                    e2sar_hip_reas *r, int force, void *stream);
/* Streaming form of recycle: move every in-progress event (its table entry and the
 * bytes received so far) to the alternate table/arena, which becomes current; the old
 * arena is free again.  Needs E2SAR_HIP_REAS_COMPACTABLE, and every completed record
 * polled (their arena offsets refer to the old arena; copy the bytes out first).
 * Asynchronous; e2sar_hip_reas_arena() returns the new base afterwards. */
int e2sar_hip_reas_compact(e2sar_hip_reas *r, void *stream);
/* Zero the statistics counters (event counters, per-datagram counters, error flags).
 * Completed and lost records not yet polled stay queued.  Asynchronous. */
int e2sar_hip_reas_reset_stats(e2sar_hip_reas *r, void *stream);

/* ------------------------------------------------------------------ */
/* device-side delivery: completed events leave the reassembler without the host.  The  */
/* batch form of getEvent's out-params (e2sarDPReassembler.cpp:626-641) with the bytes  */
/* staying in HBM: it replaces the poll -> host span table -> e2sar_hip_copy_spans      */
/* round trip for a consumer that runs on the same GPU.                                 */

/* One taken event: where its bytes sit in d_out.  32 bytes. */
typedef struct e2sar_hip_collect_rec {
    uint64_t eventNum;
    uint64_t outOffset;     /* byte offset of the event in d_out */
    uint32_t bytes;         /* the event's full length, also when truncated */
    uint16_t dataId;
    uint16_t flags;         /* E2SAR_HIP_COLLECT_* */
    uint32_t numFragments;
    uint32_t reserved;      /* the library's (the event's first 8-KiB copy piece); callers do not read it */
} e2sar_hip_collect_rec;
/* row mode: the event is longer than the pitch, its row holds the first `pitch` bytes */
#define E2SAR_HIP_COLLECT_TRUNCATED 1u

/* Pack completed records [firstRecord, firstRecord + avail) -- avail = min(records        */
/* completed, queueCapacity) - firstRecord, 0 if that is negative: the cursor rule of      */
/* e2sar_hip_relay_plan -- into d_out (device, outBytes bytes, 256-byte aligned), in        */
/* record order, and describe them in d_index[0, n) (device, maxEvents entries).          */
/*   pitch == 0, ragged: event i at the sum over j < i of bytes_j rounded up to `align`   */
/* (a power of two in [16, 4096]; 0 = 256).  Taken: the longest prefix of the records     */
/* with i < maxEvents whose every event ends inside outBytes; nothing after the first     */
/* event that does not fit is taken.  Only the events' own bytes are written: the padding */
/* between events and everything after the last keep what they held.                       */
/*   pitch > 0 (a multiple of 16), rows: n = min(avail, maxEvents, outBytes / pitch);      */
/* event i at i * pitch, min(bytes, pitch) bytes copied, the rest of the row zeros, flags */
/* TRUNCATED where bytes > pitch; rows >= n keep what they held.  `align` is ignored.  A   */
/* d_out of n rows is a [n, pitch] byte tensor.                                             */
/*   d_counts (device, 4 entries): [0] = n; [1] = bytes of d_out spanned (the last        */
/* event's offset + its length rounded up to `align`; n * pitch; 0 when n == 0); [2] =     */
/* avail - n, the records left for a call with firstRecord + n; [3] = event bytes copied. */
/* outBytes == 0 is legal (n = 0).  All offsets are 64-bit.                                 */
/*   The records stay queued: a later poll returns them, recycle discards them.  The      */
/* caller orders the call after the reassembly launches whose events it wants (the same  */
/* stream, or an event).  The bytes in d_out are a copy: recycle or compact may follow as */
/* soon as the collect has run on the stream.  Two kernel launches, no allocation, no      */
/* memset node, no wait: the call may be captured into a HIP graph.  Asynchronous.        */
int e2sar_hip_reas_collect(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxEvents,
                           uint8_t *d_out, uint64_t outBytes, uint32_t pitch, uint32_t align,
                           e2sar_hip_collect_rec *d_index, uint64_t *d_counts, void *stream);

/* ------------------------------------------------------------------ */
/* a receive graph that runs without end: reassemble_batch_dev -> collect_next -> turn,     */
/* captured once, replayed over a stream whose events begin in one replay and end in a      */
/* later one, with no host read.  collect_next is getEvent (e2sarDPReassembler.cpp:626-641) */
/* behind a cursor the device keeps; turn is the upkeep a host loop does between batches -- */
/* the poll + recycle/compact round trip of csrc/host/reassembler.cpp:504 and the GC pass   */
/* of e2sarDPReassembler.cpp:236-291 -- decided and done on the device.                     */

/* e2sar_hip_reas_collect with firstRecord = *d_cursor, a device uint32 the caller owns and */
/* zeroes once: the plan launch reads it when it runs, and leaves it grown by d_counts[0].   */
/* It does not move for a record that was not taken.  Everything else is collect's contract */
/* to the letter, ragged and rows: the taken prefix, the bytes written and never written,   */
/* d_counts[0..3], the statuses, two launches with no allocation, memset node or wait.      */
/* outBytes == 0 takes nothing and leaves the cursor where it was; d_cursor == NULL is      */
/* E2SAR_HIP_ERR_PARAMETER.                                                                  */
/*   A host e2sar_hip_reas_poll slides the record list down, after which the cursor no      */
/* longer means anything: a reassembler consumed through a cursor is not polled, unless the */
/* caller re-zeroes the cursor after a poll that drained the list.  e2sar_hip_reas_turn      */
/* zeroes it together with the list.  Asynchronous; may be captured into a HIP graph.       */
int e2sar_hip_reas_collect_next(e2sar_hip_reas *r, uint32_t *d_cursor, uint32_t maxEvents,
                                uint8_t *d_out, uint64_t outBytes, uint32_t pitch, uint32_t align,
                                e2sar_hip_collect_rec *d_index, uint64_t *d_counts, void *stream);

/* When a turn runs, and how long it carries an event in progress. */
typedef struct e2sar_hip_turn_marks {
    uint64_t arenaMark;    /* run when arena bytes in use >= this */
    uint32_t recordMark;   /* ... or completed records stored >= this */
    uint32_t tableMark;    /* ... or table slots ever claimed this epoch >= this */
    uint32_t maxCarries;   /* an event already carried this many times is lost, not carried */
    uint32_t reserved;     /* 0 */
} e2sar_hip_turn_marks;

/* Upkeep decided on the device when the launches run, that keeps the events in progress.   */
/* d_status (device, 4 entries): [0] the verdict, [1] survivors carried, [2] events aged    */
/* out, [3] arena bytes in use afterwards; a skipped turn leaves [1] = [2] = 0 and [3] the  */
/* current use.                                                                              */
/*   [0] = 2, skipped: *d_cursor < min(records completed, queueCapacity) -- a record has    */
/* not been collected, and unconsumed records point into the arena, which must not move     */
/* under them.  Nothing changes.                                                             */
/*   [0] = 0, skipped: none of the marks is reached.  Nothing changes.  Arena bytes in use  */
/* is the arena's top, above arenaBytes once it overflowed; tableMark compares against the  */
/* live tableUsed of e2sar_hip_reas_get_stats.  A mark of 0 is always reached: all-zero     */
/* marks run every time.                                                                     */
/*   [0] = 1, ran.  Every event in progress carried fewer than maxCarries times is still in */
/* progress -- key, length, bytes and fragments received, first-fragment time all kept, its */
/* carry count one higher -- and later fragments complete it to the bytes a reassembler     */
/* never turned would deliver; one created without a buffer (arena full) stays without, as  */
/* e2sar_hip_reas_compact leaves it.  Every other event in progress is lost as the GC pass  */
/* loses one: reassemblyLoss + 1, inProgress - 1, a lost record {eventNum, numFragments,    */
/* dataId, enqueueLoss = 0} if the list has room; maxCarries = 0xFFFFFFFF never loses one.  */
/* The completed list is empty and *d_cursor = 0; arena use is the survivors' lengths, each */
/* rounded up to 256 (a zero length takes 256); tableUsed is their number, the entries of   */
/* finished and lost events are gone.  The history counters, the per-datagram counters, the */
/* lost list and errorFlags keep their values.  e2sar_hip_reas_arena() returns the base it  */
/* returned before: a graph captured earlier, or holding the turn, still points at the      */
/* right memory.                                                                             */
/*   The carry count is the clock: now_ms is a host argument of every reassembly launch,    */
/* frozen in a replayed graph, so a timeout against it would mean nothing there.  A caller  */
/* who replays at a known cadence converts the timeout to turns; e2sar_hip_reas_gc still    */
/* does GC by time outside graphs.                                                           */
/*   E2SAR_HIP_ERR_PARAMETER for a NULL r, d_cursor, marks or d_status or a non-zero        */
/* reserved; E2SAR_HIP_ERR_LOGIC for a reassembler created without                           */
/* E2SAR_HIP_REAS_COMPACTABLE (the survivors pass through the alternate table and arena) or */
/* with E2SAR_HIP_REAS_REFERENCE_ORDER (a key's slot is reused there for its next item,     */
/* which a count per slot would age).  A failing call launches nothing.  Four launches      */
/* whatever the device decides, grids from tableSlots alone; no allocation, no memset node, */
/* no wait, no read-back: the call may be captured into a HIP graph.  A host                */
/* e2sar_hip_reas_compact between the capture and a replay of any launch of this            */
/* reassembler invalidates the graph, as it always did.  Asynchronous.                      */
int e2sar_hip_reas_turn(e2sar_hip_reas *r, uint32_t *d_cursor, const e2sar_hip_turn_marks *marks,
                        uint64_t *d_status /* device, 4 entries */, void *stream);

/* ------------------------------------------------------------------ */
/* device-side event building: the completed records of one window, sorted by (eventNum,  */
/* dataId) and grouped into built events -- every source's buffer for one eventNum side by */
/* side, which is what a receiver behind an EJFAT load balancer works on.  The batch form */
/* of getEvent's out-params (e2sarDPReassembler.cpp:626-641), grouped: it replaces the     */
/* collect -> host sort and group -> span table -> e2sar_hip_copy_spans round trip.  It   */
/* sits beside e2sar_hip_reas_collect, which delivers in completion order.                 */

#define E2SAR_HIP_BUILD_MAX_RECORDS 4096u   /* records one call can look at */
#define E2SAR_HIP_BUILD_MAX_IDS 64u         /* dataIds one call can name */
/* e2sar_hip_built_rec.flags: ids were given and at least one of them is absent */
#define E2SAR_HIP_BUILT_INCOMPLETE 1u

/* One built event: the members d_members[firstMember, firstMember + nMembers).  32 bytes. */
typedef struct e2sar_hip_built_rec {
    uint64_t eventNum;
    uint64_t presentMask;  /* ids given: bit j set iff dataIds[j] is present; else 0 */
    uint64_t outOffset;    /* ragged: its first member's offset; cells: g * nIds * pitch */
    uint32_t firstMember;  /* index of its first member in d_members */
    uint16_t nMembers;
    uint16_t flags;        /* E2SAR_HIP_BUILT_* */
} e2sar_hip_built_rec;

/* Build the window of completed records [firstRecord, firstRecord + W) -- W = min(avail,  */
/* maxRecords), avail by collect's cursor rule -- into d_out (device, outBytes bytes,       */
/* 256-byte aligned).  All arithmetic is 64-bit.                                             */
/*   Eligible: with nIds == 0 every record; else the records whose dataId is in dataIds    */
/* (host array of nIds distinct ids, read at call time), the rest are foreign: skipped and */
/* counted.  Among eligible records of equal (eventNum, dataId) the one completed first is  */
/* the member, the others are duplicates: skipped and counted (under REFERENCE_ORDER a     */
/* full replay of an event completes a second record).                                      */
/*   Order: the members ascend by eventNum (unsigned 64-bit), then by the id's position j  */
/* in dataIds, without ids by dataId: the result does not depend on the completion order.  */
/* A group is a maximal run of members with one eventNum; the window holds G groups, and a */
/* group is taken whole or not at all.                                                      */
/*   pitch == 0, ragged: the members in order, each at the sum of the earlier members'     */
/* lengths rounded up to `align` (collect's rule: a power of two in [16, 4096]; 0 = 256).  */
/* Taken: the longest prefix of groups with g < maxGroups whose every member ends inside  */
/* outBytes.  Only the members' own bytes are written.                                      */
/*   pitch > 0 (a multiple of 16; nIds >= 1), cells: n = min(G, maxGroups, outBytes /      */
/* (nIds * pitch)); group g at g * nIds * pitch, its cell j at + j * pitch.  A present     */
/* cell holds min(bytes, pitch) event bytes, then zeros up to the pitch, its member flags  */
/* E2SAR_HIP_COLLECT_TRUNCATED where bytes > pitch; an absent cell is pitch zeros.  A d_out */
/* of n groups is a [n, nIds, pitch] byte tensor.  `align` is checked and otherwise ignored. */
/*   Never written: bytes outside the taken groups' extents (the padding between ragged   */
/* members included), d_members entries at or past d_counts[1], d_groups entries at or      */
/* past d_counts[0].                                                                         */
/*   d_members (device, maxRecords entries): member m as collect describes an event --     */
/* outOffset, bytes, dataId, flags, numFragments; `reserved` is the library's.  d_groups   */
/* (device, maxGroups entries): the groups taken.  d_counts (device, 8 entries): [0] groups */
/* taken; [1] members taken; [2] bytes of d_out spanned (ragged: the last member's offset + */
/* its padded length; cells: n * nIds * pitch; 0 when nothing is taken); [3] event bytes    */
/* copied; [4] W; [5] duplicates skipped and [6] foreign records skipped, both over the    */
/* whole window; [7] G - n.  outBytes == 0 is legal and takes nothing: [4]-[7] are filled. */
/*   d_work: device scratch of the caller, 256-byte aligned, at least                       */
/* e2sar_hip_reas_build_work_bytes(maxRecords) bytes (0 for a maxRecords out of range), no  */
/* initialisation; it carries the plan to the copy, and is free again when the call has    */
/* run on the stream.                                                                        */
/*   The records stay queued, as for collect; the bytes in d_out are a copy.  Two kernel   */
/* launches (one when there is no room for any byte), no allocation, no memset node, no     */
/* wait: the call may be captured into a HIP graph.  Asynchronous.                          */
/*   Status: PARAMETER for a NULL r, d_out, d_members, d_groups, d_counts or d_work,       */
/* maxRecords 0 or above E2SAR_HIP_BUILD_MAX_RECORDS, maxGroups 0, nIds above               */
/* E2SAR_HIP_BUILD_MAX_IDS, nIds > 0 with NULL dataIds, a repeated id, pitch > 0 with nIds  */
/* == 0, a pitch that is no multiple of 16, a bad align, d_out or d_work not 256-byte       */
/* aligned, workBytes too small; OUT_OF_RANGE when the copy launch would exceed 2^31 - 1    */
/* workgroups.  A failing call launches nothing.                                            */
size_t e2sar_hip_reas_build_work_bytes(uint32_t maxRecords);
int e2sar_hip_reas_build(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxRecords,
                         const uint16_t *dataIds, uint32_t nIds,
                         uint8_t *d_out, uint64_t outBytes, uint32_t pitch, uint32_t align,
                         e2sar_hip_collect_rec *d_members,
                         e2sar_hip_built_rec *d_groups, uint32_t maxGroups,
                         uint64_t *d_counts,
                         void *d_work, size_t workBytes, void *stream);

/* ------------------------------------------------------------------ */
/* relay (BASELINE config 5: receive -> reassemble -> segment -> send on one GPU): the    */
/* events a reassembler completed are segmented again without a host round trip.  The  */
/* Segmenter's per-event rules (numbering, dataId, entropy, LB tick: cpp:707-728,      */
/* 901-948) are replaced by: RE eventNum and dataId as received, one LB tick for the   */
/* batch, entropy of the i-th planned event = entropyBase + i (mod 2^16).               */

/* Completed records [firstRecord, firstRecord + n) -- n = min(maxEvents, records the    */
/* reassembler holds past firstRecord) -- become seg descriptors d_events[0, n) (device, */
/* maxEvents entries) with pktBase filled in; d_counts[0] = n, d_counts[1] = their       */
/* datagram count (device, 2 entries).  The event bytes stay in the arena: recycle or    */
/* compact only after the segmentation that reads them.  Asynchronous.                  */
int e2sar_hip_relay_plan(e2sar_hip_reas *r, uint32_t firstRecord, uint32_t maxEvents, size_t maxPldLen,
                         uint64_t lbTick, uint16_t entropyBase, e2sar_hip_seg_event *d_events,
                         uint32_t *d_counts, void *stream);
/* e2sar_hip_segment_batch with the event count read on the device (d_counts[0], as     */
/* e2sar_hip_relay_plan writes it); maxEvents bounds it.  Event data 256-byte aligned    */
/* (arena buffers), so the dword-aligned path is used when maxPldLen % 4 == 0.           */
int e2sar_hip_segment_batch_dev(e2sar_hip_ctx *ctx, const e2sar_hip_seg_event *d_events,
                                const uint32_t *d_counts, uint32_t maxEvents, uint32_t maxPacketsPerEvent,
                                int lbHdrVersion, uint32_t maxPldLen, uint8_t *d_packets, uint32_t stride,
                                uint32_t *d_lens, void *stream);

/* ------------------------------------------------------------------ */
/* device-side production: events a kernel on the same GPU produced are segmented      */
/* without the host knowing their count, lengths or offsets.  Replaces, for a batch,   */
/* the _send loop (e2sarDPSegmenter.cpp:660-871) and, on the device, the Segmenter's   */
/* per-event rules the host applies in front of it (cpp:707-728, 901-948).  The send-  */
/* side mirror of e2sar_hip_reas_collect.                                              */

/* Where the events lie.  Event i has d_bytes[i] bytes.                                 */
/*   pitch > 0, rows: event i at d_data + i * pitch; d_offsets must be NULL.            */
/*   pitch == 0, ragged: event i at d_data + d_offsets[i] (device u64 array).           */
/* Available events: min(*d_count, maxEvents), or maxEvents when d_count is NULL; in    */
/* row mode also at most dataBytes / pitch.  Any address alignment is legal (the kernel */
/* picks its dword or byte path per event).  maxEventBytes: a hint for ragged events, an */
/* upper bound of their lengths (0 = unknown); it selects a kernel instantiation only,  */
/* results do not depend on it.  48 bytes.                                              */
typedef struct e2sar_hip_seg_source {
    const uint8_t *d_data;     /* device region the events lie in */
    uint64_t dataBytes;        /* its size */
    const uint32_t *d_bytes;   /* device u32[maxEvents]: event lengths */
    const uint32_t *d_count;   /* device u32, or NULL */
    const uint64_t *d_offsets; /* device u64[maxEvents] (ragged), or NULL (rows) */
    uint32_t pitch;
    uint32_t maxEventBytes;
} e2sar_hip_seg_source;

/* How the events are numbered (the host rules of cpp:707-728 and 901-948, per event i   */
/* of the source): RE eventNum = d_eventNums[i] if that device array is given, else      */
/* eventNumBase + i (64-bit wrap); lbTick = lbTickBase + i * lbTickStep; dataId constant; */
/* entropy = entropyBase + i (mod 2^16), e2sar_hip_relay_plan's rule; with               */
/* E2SAR_HIP_SEG_TICKS_AS_EVENTNUM the RE eventNum is the event's lbTick (cpp:723-724). */
/* 40 bytes.                                                                             */
typedef struct e2sar_hip_seg_numbering {
    const uint64_t *d_eventNums;   /* device u64[maxEvents], or NULL */
    uint64_t eventNumBase;
    uint64_t lbTickBase;
    uint64_t lbTickStep;
    uint16_t dataId;
    uint16_t entropyBase;
    uint32_t flags;                /* E2SAR_HIP_SEG_* */
} e2sar_hip_seg_numbering;
#define E2SAR_HIP_SEG_TICKS_AS_EVENTNUM 1u

/* Plan and segment the source's events in one call: two kernel launches, no allocation,  */
/* no memset node, no wait -- the call may be captured into a HIP graph.                  */
/*   Taken: the longest prefix of the available events in which (a) every event's bytes   */
/* lie inside the source -- rows: bytes <= pitch; ragged: offset + bytes <= dataBytes, in */
/* 64 bits -- and (b) all datagrams fit in maxPackets slots.  Nothing after the first     */
/* event that fails either test is taken, even if it would fit.  No byte of an event that */
/* was not taken is read.                                                                 */
/*   d_counts (device, 8 entries): [0] = n taken; [1] = their datagram count; [2] =       */
/* available - n; [3] = why the prefix ended: 0 all taken, 1 packet capacity, 2 an event  */
/* outside its source (also: rows the count names lie past dataBytes); [4] the library's  */
/* (the unit total the copy launch reads); [5..7] reserved.                               */
/*   d_events[0, n) (device, maxEvents entries): the descriptors e2sar_hip_seg_plan would */
/* produce for the same lengths (pktBase the exclusive prefix of ceil(bytes/maxPldLen), an */
/* empty event has no datagram), except `reserved`, which is the library's.  Entries at   */
/* or past n, and slots and d_lens entries at or past d_counts[1], keep what they held.   */
/*   Datagram bytes, zero fill and d_lens (optional): e2sar_hip_segment_batch's contract. */
/* Status: PARAMETER for a NULL required pointer, pitch and d_offsets both set or neither, */
/* maxPldLen 0 or above a UDP datagram, a bad stride, unknown flags; OUT_OF_RANGE when     */
/* maxPackets * (stride / 16) exceeds 2^32 - 1 or the launch would exceed 2^31 - 1         */
/* workgroups.  maxEvents == 0 succeeds with nothing launched.  Asynchronous.             */
int e2sar_hip_seg_emit(e2sar_hip_ctx *ctx, const e2sar_hip_seg_source *src,
                       const e2sar_hip_seg_numbering *num, uint32_t maxEvents,
                       int lbHdrVersion, uint32_t maxPldLen,
                       uint8_t *d_packets, uint32_t stride, uint32_t maxPackets, uint32_t *d_lens,
                       e2sar_hip_seg_event *d_events, uint32_t *d_counts, void *stream);

/* ------------------------------------------------------------------ */
/* Reassembly straight into a tensor.  A stream that numbers its events consecutively    */
/* (the Segmenter's default rule, e2sarDPSegmenter.cpp:901-948) and names its sources by  */
/* dataId needs no event table, no arena and no second copy: the place of a fragment in a */
/* dense [nEvents, nIds, pitch] byte tensor follows from its header alone -- row eventNum */
/* mod nEvents, cell j where dataIds[j] == dataId, byte bufferOffset.  The family below   */
/* is stateless, as e2sar_hip_seg_emit is: there is no e2sar_hip_reas object, every piece */
/* of state is device memory the caller owns, and the descriptor is a host struct read    */
/* when a call is made.  It replaces the per-packet body of the receive thread,           */
/* e2sarDPReassembler.cpp:335-427 (header validation, eventsInProgress lookup and insert, */
/* the memcpy at 391, the completion test at 403), the event queue behind it and -- with  */
/* e2sar_hip_rows_advance -- the garbage collection of events that never complete         */
/* (cpp:283-308).                                                                         */
/*   The window is a ring: it holds the events eventNum in [*d_base, *d_base + nEvents),  */
/* and e2sar_hip_rows_advance moves it on.  The chain producer -> e2sar_hip_seg_emit ->   */
/* e2sar_hip_rows_reassemble -> consumer -> e2sar_hip_rows_advance is one capturable      */
/* chain with no host read, and it runs without end.                                      */
/*   A cell (16 bytes, 16-byte aligned) is the state of one (event, source): `acc` has    */
/* the event table's accumulator layout, curBytes in the low 36 bits and the fragment     */
/* count above; `bytes` is the event's length S, the bufferLength of the fragment that    */
/* opened the cell (0 = empty: nothing arrived); `flags` says whether the cell is         */
/* COMPLETE (curBytes reached S) and whether a fragment passed the pitch (TRUNCATED: its  */
/* bytes past the pitch were dropped, but counted).  The cell of (eventNum, dataIds[j])   */
/* is c = (eventNum & (nEvents - 1)) * nIds + j, its bytes start at d_out + c * pitch     */
/* (64-bit arithmetic throughout).  The consumer reads `bytes` and `flags` of a cell and  */
/* then the first min(bytes, pitch) bytes of its row; the rest of the row is never        */
/* written and keeps what it held.                                                        */
/*   d_counts (device u64[16], accumulating): [0] cells completed, [1] fragments          */
/* accepted, [2] their payload bytes, [3] late (behind the window), [4] early (ahead of   */
/* it), [5] foreign dataId, [6] bad header, [7] data error, [8] cells released incomplete */
/* by advance, [9] cells released complete, [10] datagrams of events the window does not   */
/* own (a lattice only, below); [11] duplicates (the seen calls only, below); [12..15]      */
/* reserved, written only by clear.                                                       */
/*   The lattice.  Events are sharded over W consumers by eventNum mod W (the multi-GPU    */
/* section below); the window of consumer r holds its share, not every event number.      */
/* With eventStep = S > 1 and eventPhase = P < S, position i of the window holds event    */
/* *d_base + i * S, where *d_base mod S == P.  Let q(ev) = ev / S (floor) and owned(ev)   */
/* <=> ev mod S == P: wherever this family says eventNum of a row, a distance or the      */
/* window's extent, read q(eventNum) -- the row of an owned event is q(ev) & (nEvents -   */
/* 1), its distance from the base q(ev) - q(*d_base), and the window holds the nEvents    */
/* owned events from *d_base on.  *d_base itself stays an event number.  kMax, slack, k   */
/* and the horizon H of the calls below count window positions, that is owned events,     */
/* not raw event numbers.  q is exact for every 64-bit eventNum and every S < 2^32.       */
/* Event numbers do not wrap on a lattice: a stream is assumed to stay below 2^64 -       */
/* nEvents * S.  eventStep 0 or 1 is the consecutive window, bit for bit, with its 64-bit */
/* wrap; eventPhase must then be 0.                                                       */
#define E2SAR_HIP_ROWS_MAX_IDS 64u
#define E2SAR_HIP_ROWS_COMPLETE 1u
#define E2SAR_HIP_ROWS_TRUNCATED 2u
typedef struct e2sar_hip_rows_cell {   /* 16 bytes */
    uint64_t acc;     /* curBytes (low 36 bits) | fragments << 36 */
    uint32_t bytes;   /* the event's length S; 0 = empty */
    uint32_t flags;   /* E2SAR_HIP_ROWS_COMPLETE, E2SAR_HIP_ROWS_TRUNCATED */
} e2sar_hip_rows_cell;

typedef struct e2sar_hip_rows {
    uint8_t *d_out;               /* [nEvents, nIds, pitch] bytes, 256-byte aligned */
    e2sar_hip_rows_cell *d_cells; /* [nEvents * nIds], 16-byte aligned */
    uint64_t *d_base;             /* device u64: the window is eventNum in [base, base + nEvents) */
    uint64_t *d_counts;           /* device u64[16], accumulating */
    const uint16_t *dataIds;      /* host array, nIds distinct ids, 1..64 */
    uint32_t nIds;
    uint32_t nEvents;             /* power of two */
    uint32_t pitch;               /* multiple of 256 */
    int withLBHeader;
    uint32_t eventStep;           /* 0 or 1: consecutive events; S > 1: position i holds event base + i * S */
    uint32_t eventPhase;          /* < max(eventStep, 1): the window's events have eventNum mod S == eventPhase */
} e2sar_hip_rows;                 /* 64 bytes */

/* The datagrams [0, n) of a batch into the window, n = min(*d_count, maxPackets), or     */
/* maxPackets when d_count is NULL.  Slots and lengths: e2sar_hip_reassemble_batch's      */
/* conventions.  One kernel launch, no allocation, no memset node, no wait and nothing    */
/* read back: the call may be captured into a HIP graph.  The launch's geometry comes     */
/* from maxPackets; no byte of a slot and no d_lens entry at or past n is read.           */
/*   Per datagram, the first rule that applies:                                           */
/*   1. header: the validation of e2sar_hip_reassemble_batch (cpp:340-357): a bad RE      */
/*      version or a datagram too short for its headers -> counts[6]; a datagram longer   */
/*      than its slot -> counts[7];                                                       */
/*   1b. (eventStep > 1) an event the window does not own, eventNum mod S != P ->        */
/*      counts[10]; such a datagram costs its header read only: no wave loads its payload;*/
/*   2. a dataId that is not in dataIds -> counts[5];                                     */
/*   3. window: d = eventNum - *d_base (64-bit wrap; on a lattice q(eventNum) -           */
/*      q(*d_base)); d >= nEvents -> counts[3] (late) when (int64_t)d < 0, else counts[4] */
/*      (early);                                                                          */
/*   4. own bounds: bufferLength == 0, or bufferOffset + payload > bufferLength (64 bits) */
/*      -> counts[7]; such a fragment opens no cell;                                      */
/*   5. the cell's length S is its `bytes` if that is not 0; otherwise this fragment      */
/*      opens the cell with bytes = bufferLength (a compare-and-swap against 0: exactly   */
/*      one opener wins).  bufferOffset + payload > S -> counts[7];                       */
/*   6. accepted: payload bytes [0, min(payload, max(0, pitch - bufferOffset))) are       */
/*      written at the cell's bufferOffset; bufferOffset + payload > pitch sets           */
/*      TRUNCATED; acc grows by (payload, 1 fragment), the payload in full even where it  */
/*      was cut; counts[1] += 1, counts[2] += payload; an add of more than 0 bytes that   */
/*      brings curBytes to exactly S sets COMPLETE and adds 1 to counts[0].               */
/* A datagram stopped by rules 1-5 writes nothing and touches no cell.  Never written:    */
/* bytes of d_out outside the accepted fragments' (cut) extents, counts[8..9] and         */
/* counts[11..15], and counts[10] by a consecutive window.                                */
/*   Consecutive datagrams of one cell may be added as one.  The result does not depend   */
/* on the order of the datagrams nor on how a stream is cut into batches, provided no     */
/* fragment arrives twice and each cell has one determinate opener within a launch (all   */
/* its fragments in the launch announce one length, or the cell was opened by an earlier  */
/* launch).  Unlike the reference, an offset-0 fragment is not special, a bufferLength of */
/* 0 is a data error, and nothing is logged as lost: see e2sar_hip_rows_advance.  A       */
/* stream that may repeat a fragment goes through e2sar_hip_rows_reassemble_seen (below). */
/*   Flags and lengths are for launches ordered after this one.                           */
/* Status: PARAMETER for a NULL ctx, w, d_packets or d_lens, a NULL d_out, d_cells,       */
/* d_base, d_counts or dataIds, nIds 0 or above 64 or a repeated id, nEvents 0 or not a   */
/* power of two, pitch 0 or not a multiple of 256, d_out not 256-byte aligned, d_cells    */
/* not 16-byte or d_base / d_counts not 8-byte aligned, eventPhase >= max(eventStep, 1),  */
/* a stride or packet pointer e2sar_hip_reassemble_batch refuses; OUT_OF_RANGE when       */
/* nEvents * nIds exceeds 2^32 - 1, maxPackets * (stride / 16) exceeds 2^32 - 1 or the    */
/* launch would exceed 2^31 - 1 workgroups.  maxPackets == 0 succeeds with nothing        */
/* launched; a failing call launches nothing.  Asynchronous.                              */
int e2sar_hip_rows_reassemble(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const uint8_t *d_packets,
                              uint32_t stride, const uint32_t *d_lens, const uint32_t *d_count,
                              uint32_t maxPackets, void *stream);

/* The ring's upkeep, decided on the device: k = min(*d_k, kMax, nEvents), or min(kMax,   */
/* nEvents) when d_k is NULL.  For each of the k oldest events, base .. base + k - 1 (on a */
/* lattice the k oldest positions, base, base + S, .. base + (k - 1) * S), and            */
/* every id: a cell with bytes != 0 and no COMPLETE adds 1 to counts[8] -- the loss a     */
/* garbage-collection pass of the reference would log (cpp:283-308) -- a COMPLETE cell    */
/* adds 1 to counts[9], and the cell is zeroed; row bytes are not touched.  Then *d_base  */
/* += k (64-bit wrap; on a lattice k * S).  k == 0 changes nothing.  Two launches, their grids from nEvents * */
/* nIds and kMax alone; capturable as above.  Status: PARAMETER as above (ctx, w and the  */
/* descriptor).  Asynchronous.                                                            */
int e2sar_hip_rows_advance(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const uint32_t *d_k,
                           uint32_t kMax, void *stream);

/* Every cell and all 16 counts zeroed, *d_base = eventBase; row bytes are not touched.   */
/* One launch of plain stores (no memset node), capturable.  Status as above, and         */
/* PARAMETER for an eventBase with eventBase mod eventStep != eventPhase (eventStep > 1). */
int e2sar_hip_rows_clear(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, uint64_t eventBase, void *stream);

/* The seen calls: a window that survives duplicates.  The calls above complete a cell    */
/* when curBytes reaches S, and a fragment that arrives twice is added twice: a duplicate */
/* together with a lost fragment of the same length marks a cell COMPLETE with a hole in  */
/* its row, and a duplicate alone makes curBytes pass S, so that the event never          */
/* completes.  The three calls below keep one bit per fragment of a cell beside the       */
/* window and take every fragment once.  The sender cuts an event into fragments of       */
/* fragBytes payload bytes (the Segmenter's maxPld; the last may be shorter), so fragment */
/* f = bufferOffset / fragBytes, exact for every 32-bit offset and every fragBytes.  The  */
/* bits are the caller's, as the rest of the window is: e2sar_hip_rows_seen_bytes(nEvents,*/
/* nIds, maxFrags) = nEvents * nIds * maxFrags / 8 bytes of device memory, 16-byte        */
/* aligned, maxFrags bits per cell, the bits of cell c from word c * maxFrags / 32, bit f */
/* of a cell in its word f / 32 at 1 << (f % 32).  maxFrags is independent of the pitch:  */
/* an event longer than the pitch still completes, TRUNCATED, if maxFrags * fragBytes     */
/* covers it.                                                                             */
/*   e2sar_hip_rows_reassemble_seen is e2sar_hip_rows_reassemble to the letter, on a      */
/* consecutive window or a lattice, with two more rules:                                  */
/*   4b. (with rule 4: the fragment's own header, it opens no cell) for a fragment of     */
/*      more than 0 payload bytes: bufferOffset mod fragBytes != 0, payload > fragBytes   */
/*      or f >= maxFrags -> counts[7];                                                    */
/*   5b. (after rule 5) for a fragment of more than 0 payload bytes: if bit f of the cell */
/*      is set, the datagram is a duplicate -> counts[11]; no byte of it is written, and  */
/*      acc and the flags do not move.  Otherwise the bit is set and rule 6 accepts the   */
/*      fragment.  A bit is set only by an accepted fragment.                             */
/* A fragment of 0 payload bytes is outside the grid and the bits: it is accepted as by   */
/* the plain call, sets no bit and is never a duplicate.  Of several copies of a fragment */
/* inside one launch exactly one is accepted, which one is not specified; across launches */
/* the earlier one wins, and its bytes stay in the row.                                   */
/*   The guarantee.  The accepted fragments of a cell lie on distinct positions of the    */
/* grid, each is at most fragBytes long and lies inside [0, S); so curBytes == S implies  */
/* that every byte of [0, S) was covered: a COMPLETE cell has had every byte of [0,       */
/* min(bytes, pitch)) of its row written by a fragment of that event.  The proviso "no    */
/* fragment arrives twice" of e2sar_hip_rows_reassemble is dropped for these calls; the   */
/* proviso of one determinate opener per cell within a launch stays.                      */
/*   e2sar_hip_rows_advance_seen is e2sar_hip_rows_advance, and also zeroes the bits of   */
/* every released cell, in the launch that zeroes the cell; e2sar_hip_rows_clear_seen is  */
/* e2sar_hip_rows_clear, and also zeroes the bits of every cell.  Stores only, no memset  */
/* node; the grids come from the descriptors and kMax alone.  All three calls are         */
/* capturable as their plain forms are: no allocation, no wait, nothing read back.        */
/* e2sar_hip_rows_ready reads cells only and serves either kind of window.                */
/*   counts[11] is the number of duplicates; the plain calls never write it outside       */
/* clear.  A window fed through e2sar_hip_rows_reassemble_seen is advanced and cleared by */
/* the seen calls only: the plain advance or clear leaves stale bits behind, after which  */
/* fragments of later events are taken for duplicates.  That is the caller's error and is */
/* not detected.                                                                          */
/* Status: the plain call's, and PARAMETER for a NULL seen or d_seen, fragBytes 0,        */
/* maxFrags 0 or not a multiple of 128, a d_seen that is not 16-byte aligned;             */
/* OUT_OF_RANGE where a launch would pass 2^31 - 1 workgroups (reassemble_seen: of        */
/* maxPackets; advance_seen: 256 16-byte words of the bits of min(kMax, nEvents) * nIds   */
/* cells each).                                                                           */
typedef struct e2sar_hip_rows_seen {
    uint32_t *d_seen;    /* device, e2sar_hip_rows_seen_bytes(...) bytes, 16-byte aligned: maxFrags bits per cell, cell c at word c * maxFrags / 32 */
    uint32_t fragBytes;  /* the sender's payload per datagram (the Segmenter's maxPld); > 0 */
    uint32_t maxFrags;   /* fragments tracked per cell; > 0, a multiple of 128 (a cell's bits are whole 16-byte stores) */
} e2sar_hip_rows_seen;   /* 16 bytes */

size_t e2sar_hip_rows_seen_bytes(uint32_t nEvents, uint32_t nIds, uint32_t maxFrags);
int e2sar_hip_rows_reassemble_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen,
                                   const uint8_t *d_packets, uint32_t stride, const uint32_t *d_lens,
                                   const uint32_t *d_count, uint32_t maxPackets, void *stream);
int e2sar_hip_rows_advance_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen,
                                const uint32_t *d_k, uint32_t kMax, void *stream);
int e2sar_hip_rows_clear_seen(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_seen *seen,
                              uint64_t eventBase, void *stream);

/* Which events are ready, decided on the device: the k that e2sar_hip_rows_advance takes,    */
/* so that e2sar_hip_rows_reassemble -> e2sar_hip_rows_ready -> consumer ->                  */
/* e2sar_hip_rows_advance(d_k = d_ready) is the chain above with no host read.  The batch    */
/* form of the reference's delivery of whole events and of its garbage collection by         */
/* eventTimeout_ms (e2sarDPReassembler.cpp:236-291), for a stream numbered consecutively:    */
/* the clock is distance in event numbers, not time, for the reason e2sar_hip_reas_turn      */
/* gives for its carry count -- a now_ms is frozen in a replayed graph.                      */
/*   Let N = nEvents, B = *d_base and i in [0, N): event i is B + i (64-bit wrap), its row   */
/* (B + i) & (N - 1) -- on a lattice event i is B + i * S and its row (q(B) + i) & (N - 1),  */
/* and i, H, slack, kMax and k all count positions of the window, that is owned events; open(i) are the ids whose cell has bytes != 0, present(i) those whose  */
/* cell is COMPLETE; R = requiredMask, or all nIds bits when that is 0.  The horizon H is 0  */
/* when no cell of the window is open, else 1 + the largest i with an open cell.  Per event, */
/* the first rule that applies:                                                              */
/*   1. complete: present(i) & R == R;                                                       */
/*   2. given up: i < H and H - 1 - i >= slack -- an event `slack` or more newer has opened  */
/*      a cell (slack 0: every event behind the horizon; 0xFFFFFFFF: never);                 */
/*   3. otherwise the event is waited for.                                                   */
/* k = min(kMax, N, the first i that is waited for).                                         */
/*   d_ready (device u32[8]): [0] k -- &d_ready[0] is e2sar_hip_rows_advance's d_k; [1] the  */
/* complete events among the k; [2] the given-up ones; [3] H; [4] the cells of the k events  */
/* that are COMPLETE, over all ids and not only R; [5] their cells that are open and not     */
/* COMPLETE; [6], [7] 0.                                                                     */
/*   d_events (device, min(kMax, N) records, or NULL: only the counts are written):          */
/* d_events[i], i < k, describes event B + i (B + i * S), in event order; `flags` has COMPLETE or        */
/* GIVEN_UP, and TRUNCATED when a cell of the event has E2SAR_HIP_ROWS_TRUNCATED.  The       */
/* event's cells start at row * nIds, its bytes at d_out + row * nIds * pitch.               */
/*   With E2SAR_HIP_ROWS_READY_ZERO, for every i < k and every j < nIds, required or not: a  */
/* COMPLETE cell gets bytes [min(bytes, pitch), pitch) of its row set to 0, any other cell   */
/* [0, pitch): the k rows are then exactly the bytes of whole events with zeros elsewhere, a */
/* dense tensor.  Without the flag d_out is not touched.                                     */
/*   Never written: the cells, *d_base and d_counts -- two calls with no reassembly between  */
/* them give the same answer, and advance still counts the released cells in counts[8] and   */
/* counts[9]; d_events entries at or past k; bytes of d_out other than those named above.    */
/*   The result describes the window as the launches ordered before this call left it: the   */
/* caller orders it after its e2sar_hip_rows_reassemble, and e2sar_hip_rows_advance before   */
/* the next one.  Two launches, three with the flag, their grids from the descriptor and     */
/* kMax alone; no allocation, no memset node, no wait and nothing read back: capturable.     */
/* d_work is the caller's, 256-byte aligned, at least e2sar_hip_rows_ready_work_bytes(N); it */
/* needs no initialisation and is free once the call has run.                                */
/* Status: e2sar_hip_rows_advance's (ctx, w and the descriptor); PARAMETER for a NULL rule,  */
/* d_ready or d_work, a reserved that is not 0, unknown flags, requiredMask bits at or above */
/* nIds, a work buffer that is too small or not 256-byte aligned, a d_ready that is not      */
/* 4-byte or a d_events that is not 8-byte aligned; OUT_OF_RANGE when the flag's launch      */
/* would exceed 2^31 - 1 workgroups (8-KiB pieces of min(kMax, N) * nIds cells).  kMax == 0  */
/* succeeds, writes d_ready with k = 0 and H, and zeroes nothing; a failing call launches    */
/* nothing.  Asynchronous.                                                                   */
#define E2SAR_HIP_ROWS_READY_ZERO   1u          /* rule.flags */
#define E2SAR_HIP_ROWS_EV_COMPLETE  1u          /* e2sar_hip_rows_event.flags */
#define E2SAR_HIP_ROWS_EV_GIVEN_UP  2u
#define E2SAR_HIP_ROWS_EV_TRUNCATED 4u          /* some cell of the event has TRUNCATED */

typedef struct e2sar_hip_rows_ready_rule {
    uint64_t requiredMask; /* bit j: dataIds[j] must be COMPLETE; 0 = all nIds */
    uint32_t slack;        /* give an event up once an event this many or more newer has opened a cell; 0xFFFFFFFF: never */
    uint32_t kMax;         /* at most this many events */
    uint32_t flags;        /* E2SAR_HIP_ROWS_READY_ZERO */
    uint32_t reserved;     /* 0 */
} e2sar_hip_rows_ready_rule;

typedef struct e2sar_hip_rows_event {   /* 32 bytes */
    uint64_t eventNum;
    uint64_t presentMask;  /* bit j: cell (event, dataIds[j]) is COMPLETE */
    uint64_t openMask;     /* bit j: cell's bytes != 0 */
    uint32_t row;          /* eventNum & (nEvents - 1), on a lattice q(eventNum) & (nEvents - 1): its cells start at row * nIds */
    uint32_t flags;
} e2sar_hip_rows_event;

size_t e2sar_hip_rows_ready_work_bytes(uint32_t nEvents);
int e2sar_hip_rows_ready(e2sar_hip_ctx *ctx, const e2sar_hip_rows *w, const e2sar_hip_rows_ready_rule *rule,
                         uint32_t *d_ready /* device u32[8] */, e2sar_hip_rows_event *d_events /* device [min(kMax, nEvents)], or NULL */,
                         void *d_work, size_t workBytes, void *stream);

/* ------------------------------------------------------------------ */
/* multi-GPU: events are owned by rank eventNum % world.  A rank that received       */
/* (landed) datagrams of other ranks' events routes them: this packs the batch into */
/* per-destination spans (stable order) and reports the span sizes, ready for one   */
/* all-to-all-v over RCCL.  The reference never needs this step: its load balancer  */
/* steers every fragment of an event to one receiver (e2sarDPSegmenter.hpp:231-235). */

size_t e2sar_hip_route_workspace_bytes(uint32_t nPackets, uint32_t world);
/* d_sendPackets: nPackets*stride bytes; d_sendLens: nPackets; d_counts: world entries
 * (datagrams per destination rank).  Datagrams whose RE header does not parse stay on
 * `self`.  world <= 64.  Asynchronous. */
int e2sar_hip_route_batch(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride,
                          const uint32_t *d_lens, uint32_t nPackets, int withLBHeader,
                          uint32_t world, uint32_t self, uint8_t *d_sendPackets,
                          uint32_t *d_sendLens, uint32_t *d_counts, void *d_workspace,
                          size_t workspaceBytes, void *stream);
/* Foreign-only routing: as e2sar_hip_route_batch, but datagrams this rank keeps -- owned
 * by `self`, or unparsable -- are neither packed nor counted (d_counts[self] = 0, and no
 * byte of theirs is read beyond the RE header).  They are reassembled where they landed
 * by a reassembler set to this rank's ownership (e2sar_hip_reas_set_owner), so only
 * (world-1)/world of an evenly spread batch crosses HBM twice and xGMI once.  Asynchronous. */
int e2sar_hip_route_foreign(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride,
                            const uint32_t *d_lens, uint32_t nPackets, int withLBHeader,
                            uint32_t world, uint32_t self, uint8_t *d_sendPackets,
                            uint32_t *d_sendLens, uint32_t *d_counts, void *d_workspace,
                            size_t workspaceBytes, void *stream);

/* Per-batch routing into per-rank regions, for a stream of landed batches exchanged once
 * per step: rank d's datagrams are appended to region d -- slots [d*capPerRank,
 * (d+1)*capPerRank) of d_sendPackets / d_sendLens -- after the ones already there, and
 * running[d] (device, world counters, zeroed by the caller before the first batch, e.g.
 * e2sar_hip_memset_d) grows by this batch's count for d.  One launch: each workgroup of 256
 * datagrams reserves its room with one atomic per destination, so within a batch the order
 * of a destination's datagrams is kept inside each 256-datagram block, and the blocks
 * append in the order they reserve (the order-insensitive reassembler does not care; a
 * REFERENCE_ORDER receiver takes the region order as the arrival order).  The workspace
 * arguments are unused (NULL / 0 allowed).  A datagram that would land past
 * its region is not written, but still counted: running[d] > capPerRank after the step
 * means the regions were too small.  foreignOnly: as e2sar_hip_route_foreign (this rank's
 * datagrams and unparsable ones stay here, running[self] stays 0).  Routing each batch
 * right after it landed reads it while it is still in the Infinity Cache; the step's one
 * all-to-all then sends each region's first running[d] slots.  Asynchronous. */
int e2sar_hip_route_append(e2sar_hip_ctx *ctx, const uint8_t *d_packets, uint32_t stride,
                           const uint32_t *d_lens, uint32_t nPackets, int withLBHeader,
                           uint32_t world, uint32_t self, int foreignOnly, uint8_t *d_sendPackets,
                           uint32_t *d_sendLens, uint32_t capPerRank, uint32_t *d_running,
                           void *d_workspace, size_t workspaceBytes, void *stream);

/* Ownership of a reassembler in a world of `world` ranks (1..64): from the next launch on,
 * a datagram whose RE header parses but whose eventNum % world != self belongs to another
 * rank and takes no part -- not counted in any statistic, no byte copied.  Unparsable
 * datagrams are still counted (badHeaderDiscards) here.  world = 1 (the default) takes
 * every datagram.  The receive-side counterpart of the reference's steering of every
 * fragment of an event to one receiver by eventNum (e2sarDPReassembler.hpp:224-229). */
int e2sar_hip_reas_set_owner(e2sar_hip_reas *r, uint32_t world, uint32_t self);
/* Set (cold != 0) or clear E2SAR_HIP_REAS_COLD_DATAGRAMS for the following launches: a
 * reassembler that takes both just-written and long-resident batches (e.g. datagrams
 * reassembled where they landed, then datagrams received from other ranks) tells each
 * launch how to load them. */
int e2sar_hip_reas_set_cold(e2sar_hip_reas *r, int cold);
/* Before destroying a stream that launched through this reassembler: wait for the stream's
 * work, stop tracking it and free its internal buffers (or retire them, if a launch of this
 * reassembler was ever captured).  Snapshots (poll, lost_poll, get_stats) wait for every
 * stream the reassembler launched on, so a stream must outlive the reassembler's last
 * snapshot unless it is forgotten first: HIP may hand a destroyed stream's handle to a new
 * stream.  (A snapshot that finds a handle already invalid drops it the same way.)  The
 * stream must still be alive when this is called (it is synchronised): call it, then
 * destroy the stream -- never the other way round.  No reference counterpart: the
 * reference's receive threads own their sockets for their life. */
int e2sar_hip_reas_forget_stream(e2sar_hip_reas *r, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* E2SAR_HIP_H */
