// reas_build.hpp -- device-side event building: the records a reassembler completed, sorted by (eventNum, dataId),
// grouped into built events and packed into a caller's device buffer.
#pragma once

#include "dev_access.hpp"
#include "reas_collect.hpp"

namespace e2sar_amd {

// ---------------------------------------------------------------------------------
// build: the window of completed records [first, first + W) leaves the arena sorted and
// grouped -- every source's buffer for one eventNum side by side -- ragged (pitch == 0: the
// members in order, each at the sum of the earlier lengths rounded up to `align`) or as cells
// (group g at g * nIds * pitch, its source j at + j * pitch, cut to the pitch, zero-filled up
// to it, an absent source all zeros).  Two launches, as collect: build_plan_kernel sorts the
// window, drops duplicates, cuts the groups, lays them out and writes the member table, the
// group table and the counts; build_copy_kernel moves the bytes, one 8-KiB piece per
// workgroup, on a grid the host sizes from bounds alone.

constexpr int kBuildBlock = 1024;                                     // the plan's one workgroup
constexpr uint32_t kBuildMaxRecords = E2SAR_HIP_BUILD_MAX_RECORDS;
constexpr uint32_t kBuildMaxIds = E2SAR_HIP_BUILD_MAX_IDS;
static_assert((kBuildMaxRecords & (kBuildMaxRecords - 1u)) == 0u, "the sort pads the window to a power of two");

// The caller's id list, by value in the kernel arguments: read at call time, and a captured
// launch keeps its copy.
struct BuildIds {
    uint16_t id[kBuildMaxIds];
};

// d_work: what the plan leaves for the copy beside the tables.  One 256-byte head, then the
// source of every member: its record's index in the window, and that record's place in the
// arena and length, so that a copy workgroup reaches its bytes with one load fewer in a row.
struct BuildWorkHead {
    uint32_t pieces;          // 8-KiB pieces of the copy launch
    uint32_t pad[63];
};
struct BuildSrc {
    uint64_t arenaOffset;
    uint32_t bytes;
    uint32_t rec;             // completed[firstRecord + rec]
};
static_assert(sizeof(BuildWorkHead) == 256 && sizeof(BuildSrc) == 16, "the member sources start on a 256-byte line");
__host__ __device__ constexpr uint64_t build_work_bytes(uint32_t maxRecords)
{
    return sizeof(BuildWorkHead) + (uint64_t)maxRecords * sizeof(BuildSrc);
}

// Sort key of a window record: the 64-bit eventNum in `ev`; in `lo` the second key (the id's
// position in the caller's list, or the dataId itself without a list) above the record's
// index in the window.  The index makes the order total, and the first of equal (eventNum,
// second key) neighbours is the record with the lowest index.  Foreign records and the
// padding up to the sort's power of two are all ones in both words: no record's `lo` is (its
// index is below 4096), so they sort behind every record, eventNum 2^64 - 1 included.
constexpr uint32_t kBuildLoPad = 0xFFFFFFFFu;
__device__ __forceinline__ bool build_key_less(uint64_t ea, uint32_t la, uint64_t eb, uint32_t lb)
{
    return ea < eb || (ea == eb && la < lb);
}

// block_scan_before for the plan's 16 waves: the waves' sums are read one per lane and summed
// over each 16 lanes by shuffles, instead of sixteen compares against the wave index whose
// lane masks the compiler would keep in scalar registers across every scan of the kernel.
template <typename T>
__device__ __forceinline__ T build_scan_before(const T *part, T &total)
{
    static_assert(kBuildBlock / 64 == 16, "one wave sum per lane of a 16-lane row");
    const uint32_t w = threadIdx.x & 15u;
    const T x = part[w];
    T before = w < (threadIdx.x >> 6) ? x : (T)0;
    total = x;
#pragma unroll
    for (int o = 8; o; o >>= 1) {
        before += __shfl_xor(before, o);
        total += __shfl_xor(total, o);
    }
    return before;
}

// One workgroup of 1024 threads.  (1) The window's keys go to LDS, 12 bytes a record (48 KiB
// at 4096 records): a record whose dataId is not in the list becomes padding and is counted.
// (2) A bitonic network over the next power of two sorts them.  (3) Two passes over the
// sorted keys, 1024 a step, on 64-bit carries: both find the members (a key whose left
// neighbour has another (eventNum, second key)), the group heads (another eventNum) and, by
// block-wide scans, each member's index, group, offset and first copy piece.  The first pass
// only finds the cut -- the group of the first ragged member that would end past outBytes --
// and the totals; a group is taken whole or not at all, so nothing is written before the
// number of groups taken is known.  The second pass writes the members and the heads of the
// groups taken.  (4) One thread per group taken closes it: the member count from the next
// group's first member, the presence mask from the members' list positions.
__global__ __launch_bounds__(kBuildBlock) void build_plan_kernel(ReasDev R, uint32_t first, uint32_t maxRecords,
                                                                 BuildIds ids, uint32_t nIds, uint64_t outBytes,
                                                                 uint32_t pitch, uint32_t align,
                                                                 e2sar_hip_collect_rec *__restrict__ members,
                                                                 e2sar_hip_built_rec *__restrict__ groups,
                                                                 uint32_t maxGroups, uint64_t *__restrict__ counts,
                                                                 uint8_t *__restrict__ work)
{
    constexpr int kWaves = kBuildBlock / 64;
    __shared__ uint64_t sEv[kBuildMaxRecords];
    __shared__ uint32_t sLo[kBuildMaxRecords];
    __shared__ uint16_t sFirst[kBuildMaxRecords + 1u];      // group -> its first member
    __shared__ uint8_t sPos[kBuildMaxRecords];              // member -> its id's position in the list
    __shared__ uint64_t wavePad[kWaves], waveTaken[kWaves], waveCopied[kWaves];
    __shared__ uint32_t waveMG[kWaves], wavePieces[kWaves], waveCut[kWaves];
    __shared__ uint16_t sIds[kBuildMaxIds];
    __shared__ uint32_t sW, sForeign;
    const uint32_t tid = threadIdx.x;
    BuildWorkHead *head = reinterpret_cast<BuildWorkHead *>(work);
    BuildSrc *srcOf = reinterpret_cast<BuildSrc *>(work + sizeof(BuildWorkHead));

    if (tid == 0) {
        sW = completed_window(R, first, maxRecords).taken;
        sForeign = 0;
    }
    if (tid < nIds) sIds[tid] = ids.id[tid];
    __syncthreads();
    const uint32_t W = sW;
    uint32_t N = 1;
    while (N < W) N <<= 1;

    // (1) keys
    uint32_t foreign = 0;
    for (uint32_t s = tid; s < N; s += kBuildBlock) {
        uint64_t ev = ~0ull;
        uint32_t lo = kBuildLoPad;
        if (s < W) {
            const e2sar_hip_event_rec rec = R.completed[first + s];
            uint32_t key = rec.dataId;
            if (nIds) {
                key = ~0u;
                for (uint32_t j = 0; j < nIds; j++)
                    if (sIds[j] == rec.dataId) key = j;
            }
            if (key != ~0u) {
                ev = rec.eventNum;
                lo = (key << 16) | s;
            } else {
                foreign++;
            }
        }
        sEv[s] = ev;
        sLo[s] = lo;
    }
    if (foreign) atomicAdd(&sForeign, foreign);
    __syncthreads();

    // (2) bitonic sort, ascending.  (Wave-local syncs in place of the barrier between the stages
    // at distance <= 64, which stay inside one wave's 128 keys, measured no gain: DESIGN.md 4.10.)
    for (uint32_t k = 2; k <= N; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < (N >> 1); t += kBuildBlock) {
                const uint32_t a = ((t & ~(j - 1u)) << 1) | (t & (j - 1u)), b = a | j;
                const uint64_t ea = sEv[a], eb = sEv[b];
                const uint32_t la = sLo[a], lb = sLo[b];
                const bool up = (a & k) == 0u;
                if (up ? build_key_less(eb, lb, ea, la) : build_key_less(ea, la, eb, lb)) {
                    sEv[a] = eb;
                    sLo[a] = lb;
                    sEv[b] = ea;
                    sLo[b] = la;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t nForeign = sForeign;
    const uint32_t nValid = W - nForeign;                    // sorted keys [0, nValid) are records

    // (3) the two passes
    const uint64_t cell = (uint64_t)nIds * pitch;            // bytes of one built event in cells
    uint32_t nGroups = 0, nMembers = 0, taken = 0;           // G and the members of the window; groups taken
    uint32_t cutG = ~0u;
    uint32_t pieces = 0;                                     // of the groups taken
    uint64_t spanned = 0, copied = 0;
    for (int pass = 0; pass < 2; pass++) {
        uint32_t carryM = 0, carryG = 0;
        uint64_t carryOff = 0;
        for (uint32_t b0 = 0; b0 < nValid; b0 += kBuildBlock) {
            const uint32_t s = b0 + tid;
            const bool valid = s < nValid;
            uint64_t ev = 0, pev = 0;
            uint32_t lo = 0, plo = 0;
            if (valid) {
                ev = sEv[s];
                lo = sLo[s];
                if (s) {
                    pev = sEv[s - 1u];
                    plo = sLo[s - 1u];
                }
            }
            const uint32_t key = lo >> 16, rec = lo & 0xFFFFu;
            const bool isHead = valid && (s == 0u || pev != ev);
            const bool isMember = valid && (isHead || (plo >> 16) != key);
            e2sar_hip_event_rec r{};
            if (isMember) r = R.completed[first + rec];
            const uint64_t pad = !isMember ? 0ull : pitch ? 0ull : (((uint64_t)r.bytes + align - 1u) & ~(uint64_t)(align - 1u));
            uint64_t stepPad;
            uint32_t stepMG;
            const uint32_t mg = (isMember ? 1u : 0u) | (isHead ? 0x10000u : 0u);
            const uint32_t incMG = block_scan_post(mg, waveMG);          // two scans behind one barrier
            const uint64_t incPad = block_scan_post(pad, wavePad);
            __syncthreads();
            const uint64_t off = carryOff + build_scan_before(wavePad, stepPad) + incPad - pad;
            const uint32_t beforeMG = build_scan_before(waveMG, stepMG) + incMG;
            const uint32_t m = carryM + (beforeMG & 0xFFFFu) - (isMember ? 1u : 0u);     // the member's index
            const uint32_t g = carryG + (beforeMG >> 16) - 1u;                          // the key's group
            if (pass == 0) {
                // a ragged member must end inside the buffer; cells are cut by outBytes / cell below
                const bool fails = isMember && !pitch && off + r.bytes > outBytes;
                const uint32_t cut = block_first<uint32_t, kWaves>(fails, g, waveCut);
                if (cut < cutG) cutG = cut;
            } else {
                const bool take = isMember && g < taken;
                const uint64_t extent = pitch ? (uint64_t)pitch : (uint64_t)r.bytes;
                const uint32_t np = (take && !pitch) ? collect_pieces(extent) : 0u;
                const uint64_t cp = !take ? 0ull : r.bytes < extent ? (uint64_t)r.bytes : extent;
                uint64_t stepTaken, stepCopied;
                uint32_t stepPieces;
                const uint32_t incNp = block_scan_post(np, wavePieces);  // three scans behind one barrier
                block_scan_post(take ? pad : (uint64_t)0, waveTaken);
                block_scan_post(cp, waveCopied);
                __syncthreads();
                const uint32_t before = pieces + build_scan_before(wavePieces, stepPieces);
                build_scan_before(waveTaken, stepTaken);
                build_scan_before(waveCopied, stepCopied);
                const uint64_t groupOff = pitch ? (uint64_t)g * cell : off;
                if (isMember && nIds) sPos[m] = (uint8_t)key;
                if (isHead) sFirst[g] = (uint16_t)m;
                if (take) {
                    e2sar_hip_collect_rec o;
                    o.eventNum = ev;
                    o.outOffset = pitch ? groupOff + (uint64_t)key * pitch : off;
                    o.bytes = r.bytes;
                    o.dataId = r.dataId;
                    o.flags = (uint16_t)((pitch && r.bytes > pitch) ? E2SAR_HIP_COLLECT_TRUNCATED : 0);
                    o.numFragments = r.numFragments;
                    o.reserved = before + incNp - np;                   // ragged: its first copy piece
                    members[m] = o;
                    srcOf[m] = BuildSrc{r.arenaOffset, r.bytes, rec};
                    if (isHead) {
                        groups[g].eventNum = ev;
                        groups[g].outOffset = groupOff;
                        groups[g].firstMember = m;
                    }
                }
                pieces += stepPieces;
                spanned += stepTaken;
                copied += stepCopied;
            }
            carryM += stepMG & 0xFFFFu;
            carryG += stepMG >> 16;
            carryOff += stepPad;
            __syncthreads();
        }
        if (pass == 0) {
            nMembers = carryM;
            nGroups = carryG;
            taken = nGroups < maxGroups ? nGroups : maxGroups;
            if (pitch) {
                if (outBytes / cell < taken) taken = (uint32_t)(outBytes / cell);
            } else if (cutG < taken) {
                taken = cutG;
            }
        }
    }
    if (tid == 0) sFirst[nGroups] = (uint16_t)nMembers;
    __syncthreads();

    // (4) close the groups taken
    for (uint32_t g = tid; g < taken; g += kBuildBlock) {
        const uint32_t m0 = sFirst[g], nm = sFirst[g + 1u] - m0;
        uint64_t mask = 0;
        if (nIds)
            for (uint32_t q = 0; q < nm; q++) mask |= 1ull << sPos[m0 + q];
        groups[g].presentMask = mask;
        groups[g].nMembers = (uint16_t)nm;
        groups[g].flags = (uint16_t)((nIds && nm != nIds) ? E2SAR_HIP_BUILT_INCOMPLETE : 0);
    }
    if (tid == 0) {
        if (pitch) {
            spanned = (uint64_t)taken * cell;
            pieces = taken * nIds * collect_pieces(pitch);   // below 2^31: the host checked the bound
        }
        counts[0] = taken;
        counts[1] = sFirst[taken];                           // the first member not taken, or all of them
        counts[2] = spanned;
        counts[3] = copied;
        counts[4] = W;
        counts[5] = nValid - nMembers;
        counts[6] = nForeign;
        counts[7] = nGroups - taken;
        head->pieces = pieces;
    }
}

// One workgroup per 8-KiB piece.  The grid comes from bounds, so a workgroup first reads the
// piece total build_plan_kernel left in the work buffer on the stream before it, and exits if
// it is past it.  Cells: the piece's cell by division, its group's record says whether source
// j is present and which member it is -- the members of a group are in list order, so it is
// the group's first member plus the present sources before j; an absent cell is zeros.  The
// first group record is loaded beside the total, not behind it: the grid's bound keeps its
// index below maxGroups, so the address is the caller's table whatever the plan took.
// Ragged: the member by last_prefix_le over the piece prefix (the members' `reserved`), as
// collect_copy_kernel.  The member's bytes lie where its BuildSrc says, and copy_piece moves
// them.  Arena event buffers are 256-byte aligned and every offset at least 16-byte aligned,
// so there is no unaligned form.  The loop is a guard, not the plan: the grid strides over
// what the bounds undercount.
__global__ __launch_bounds__(kBlock) void build_copy_kernel(const uint8_t *__restrict__ arena,
                                                            uint8_t *__restrict__ out, uint32_t pitch, uint32_t nIds,
                                                            const e2sar_hip_collect_rec *__restrict__ members,
                                                            const e2sar_hip_built_rec *__restrict__ groups,
                                                            const uint64_t *__restrict__ counts,
                                                            const uint8_t *__restrict__ work)
{
    const uint32_t total = reinterpret_cast<const BuildWorkHead *>(work)->pieces;
    const BuildSrc *srcOf = reinterpret_cast<const BuildSrc *>(work + sizeof(BuildWorkHead));
    uint32_t p = blockIdx.x;
    if (pitch) {
        const uint32_t perCell = collect_pieces(pitch);
        uint32_t c = p / perCell, g = c / nIds;
        uint64_t mask = groups[g].presentMask;
        uint32_t m0 = groups[g].firstMember;
        while (p < total) {
            const uint32_t j = c - g * nIds;
            uint64_t cp = 0;
            const uint8_t *src = arena;
            if ((mask >> j) & 1ull) {
                const BuildSrc s = srcOf[m0 + (uint32_t)__builtin_popcountll(mask & ((1ull << j) - 1ull))];
                cp = s.bytes < pitch ? s.bytes : pitch;
                src = arena + s.arenaOffset;
            }
            copy_piece<true>(src, out + (uint64_t)c * pitch, cp, pitch, (uint64_t)(p - c * perCell) * kCopyPiece);
            p += gridDim.x;
            if (p >= total) break;
            c = p / perCell;
            g = c / nIds;
            mask = groups[g].presentMask;
            m0 = groups[g].firstMember;
        }
        return;
    }
    if (p >= total) return;
    const uint32_t n = (uint32_t)counts[1];
    for (; p < total; p += gridDim.x) {
        const uint32_t m = last_prefix_le(p, n, [&](uint32_t i) { return members[i].reserved; });
        const BuildSrc s = srcOf[m];
        copy_piece<false>(arena + s.arenaOffset, out + members[m].outOffset, s.bytes, s.bytes,
                          (uint64_t)(p - members[m].reserved) * kCopyPiece);
    }
}

}  // namespace e2sar_amd
