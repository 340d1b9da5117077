/*
 * asan_stream.c -- the oracle's receive body over one datagram stream, as a stand-alone program.
 * TEST INFRASTRUCTURE ONLY; not part of libe2sar_oracle.so.  tests/test_reas_lengths_cpu.py
 * compiles it with e2sar_oracle.c under -fsanitize=address,undefined and runs it on streams
 * whose fragments disagree on bufferLength: the oracle must stay inside every buffer it owns.
 *
 * Stream file (little-endian): u64 stride, u64 n, u32 lens[n], u8 slots[n * stride].
 * The datagrams carry LB + RE headers.  The stream is pushed at clock 100 ms, every
 * completed event popped, one GC run at 1100 ms with a 500 ms timeout.  Output:
 *   stats <enqueueLoss> <reassemblyLoss> <eventSuccess> <totalBytes> <totalPackets>
 *         <badHeaderDiscards> <dataErrCnt> <inProgress>        (before the GC)
 *   event <eventNum> <dataId> <bytes> <numFragments> <checksum of the bytes, hex>   (pop order)
 *   lost <eventNum> <dataId> <numFragments>                                          (queue order)
 *   after <reassemblyLoss> <inProgress>                                            (after the GC)
 */
#include "e2sar_oracle.h"

#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

/* numFragments of the event last popped (e2sar_oracle.c; test access, not in the header) */
uint64_t e2o_reas_last_pop_frags(const e2o_reas *r);

/* sum of (i + 1) * byte[i] modulo 2^64: position-sensitive, and one line of numpy */
static uint64_t checksum(const uint8_t *p, size_t n)
{
    uint64_t h = 0;
    for (size_t i = 0; i < n; i++) h += (uint64_t)(i + 1) * p[i];
    return h;
}

int main(int argc, char **argv)
{
    if (argc != 2) { fprintf(stderr, "usage: %s STREAM\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint64_t hdr[2];
    if (fread(hdr, sizeof hdr[0], 2, f) != 2) { fprintf(stderr, "short header\n"); return 2; }
    const size_t stride = (size_t)hdr[0], n = (size_t)hdr[1];
    if (stride == 0 || stride > (1u << 20) || n > (1u << 24)) { fprintf(stderr, "bad geometry\n"); return 2; }
    uint32_t *lens = (uint32_t *)malloc((n ? n : 1) * sizeof *lens);
    uint8_t *slots = (uint8_t *)malloc(n ? n * stride : 1);
    if (!lens || !slots) { fprintf(stderr, "out of memory\n"); return 2; }
    if (fread(lens, sizeof *lens, n, f) != n || fread(slots, stride, n, f) != n) {
        fprintf(stderr, "short stream\n");
        return 2;
    }
    fclose(f);
    for (size_t i = 0; i < n; i++)
        if (lens[i] > stride) { fprintf(stderr, "datagram %zu longer than its slot\n", i); return 2; }

    e2o_reas *r = e2o_reas_new(1, 0);
    e2o_reas_set_time(r, 100);
    e2o_reas_push_batch(r, slots, n, stride, lens);
    e2o_reas_stats st;
    e2o_reas_get_stats(r, &st);
    printf("stats %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 "\n",
           st.enqueueLoss, st.reassemblyLoss, st.eventSuccess, st.totalBytes, st.totalPackets,
           st.badHeaderDiscards, st.dataErrCnt, st.inProgress);
    uint8_t *ev;
    size_t bytes;
    uint64_t num;
    uint16_t id;
    while (e2o_reas_pop(r, &ev, &bytes, &num, &id) == 0) {
        printf("event %" PRIu64 " %u %zu %" PRIu64 " %016" PRIx64 "\n", num, (unsigned)id, bytes,
               e2o_reas_last_pop_frags(r), checksum(ev, bytes));
        e2o_free(ev);
    }
    e2o_reas_set_time(r, 1100);
    e2o_reas_gc(r, 500);
    uint64_t frags;
    while (e2o_reas_lost_pop(r, &num, &id, &frags) == 0)
        printf("lost %" PRIu64 " %u %" PRIu64 "\n", num, (unsigned)id, frags);
    e2o_reas_get_stats(r, &st);
    printf("after %" PRIu64 " %" PRIu64 "\n", st.reassemblyLoss, st.inProgress);
    e2o_reas_free(r);
    free(slots);
    free(lens);
    return 0;
}
