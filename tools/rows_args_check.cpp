// The argument checks of the rows family (e2sar_hip_rows_reassemble / _advance / _clear), driven
// on the host alone: every call below fails its checks, and a failing call returns before it
// touches the device, so no GPU is needed.  For a sanitizer build of the host code:
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -Iinclude -Ie2sar_amd/csrc -o build/rows_args_check tools/rows_args_check.cpp \
//       e2sar_amd/csrc/sar_kernels.hip e2sar_amd/csrc/capi.cpp && build/rows_args_check
// The context is only compared with NULL before the checks fail, so a stand-in address serves.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "e2sar_hip.h"

static int g_bad = 0;

static void expect(int got, int want, const char *what)
{
    if (got != want) {
        std::printf("FAIL %s: status %d, expected %d (%s)\n", what, got, want, e2sar_hip_last_error());
        g_bad++;
    }
}

int main()
{
    alignas(256) static uint8_t mem[4096];
    e2sar_hip_ctx *ctx = reinterpret_cast<e2sar_hip_ctx *>(mem);          // never dereferenced by a failing call
    std::vector<uint16_t> ids(65);
    for (size_t k = 0; k < ids.size(); k++) ids[k] = (uint16_t)(k + 1);
    const uint16_t twice[2] = {5, 5};
    e2sar_hip_rows good{};
    good.d_out = mem;
    good.d_cells = reinterpret_cast<e2sar_hip_rows_cell *>(mem + 1024);
    good.d_base = reinterpret_cast<uint64_t *>(mem + 2048);
    good.d_counts = reinterpret_cast<uint64_t *>(mem + 2304);
    good.dataIds = ids.data();
    good.nIds = 2;
    good.nEvents = 4;
    good.pitch = 256;
    good.withLBHeader = 1;
    const uint8_t *pk = mem + 3072;
    const uint32_t *ln = reinterpret_cast<const uint32_t *>(mem + 3584);
    const int P = E2SAR_HIP_ERR_PARAMETER, R = E2SAR_HIP_ERR_OUT_OF_RANGE;

    std::vector<e2sar_hip_rows> bad;
    auto with = [&](auto edit) {
        e2sar_hip_rows w = good;
        edit(w);
        bad.push_back(w);
    };
    with([](e2sar_hip_rows &w) { w.d_out = nullptr; });
    with([](e2sar_hip_rows &w) { w.d_cells = nullptr; });
    with([](e2sar_hip_rows &w) { w.d_base = nullptr; });
    with([](e2sar_hip_rows &w) { w.d_counts = nullptr; });
    with([](e2sar_hip_rows &w) { w.dataIds = nullptr; });
    with([](e2sar_hip_rows &w) { w.nIds = 0; });
    with([](e2sar_hip_rows &w) { w.nIds = 65; });
    with([&](e2sar_hip_rows &w) { w.dataIds = twice; });
    with([](e2sar_hip_rows &w) { w.nEvents = 0; });
    with([](e2sar_hip_rows &w) { w.nEvents = 6; });
    with([](e2sar_hip_rows &w) { w.pitch = 0; });
    with([](e2sar_hip_rows &w) { w.pitch = 128; });
    with([](e2sar_hip_rows &w) { w.d_out += 128; });
    with([](e2sar_hip_rows &w) { w.d_cells = reinterpret_cast<e2sar_hip_rows_cell *>(reinterpret_cast<uint8_t *>(w.d_cells) + 8); });
    with([](e2sar_hip_rows &w) { w.eventStep = 2; w.eventPhase = 2; });        // the lattice: phase < max(step, 1)
    with([](e2sar_hip_rows &w) { w.eventStep = 0; w.eventPhase = 1; });
    with([](e2sar_hip_rows &w) { w.eventStep = 1; w.eventPhase = 1; });
    with([](e2sar_hip_rows &w) { w.eventStep = 0xFFFFFFFFu; w.eventPhase = 0xFFFFFFFFu; });
    for (const e2sar_hip_rows &w : bad) {
        expect(e2sar_hip_rows_reassemble(ctx, &w, pk, 64, ln, nullptr, 4, nullptr), P, "reassemble, bad descriptor");
        expect(e2sar_hip_rows_advance(ctx, &w, nullptr, 1, nullptr), P, "advance, bad descriptor");
        expect(e2sar_hip_rows_clear(ctx, &w, 0, nullptr), P, "clear, bad descriptor");
    }
    e2sar_hip_rows wide = good;
    wide.nIds = 64;                                                       // all 64 ids are read, none past them
    wide.nEvents = 1u << 31;
    expect(e2sar_hip_rows_reassemble(ctx, &wide, pk, 64, ln, nullptr, 4, nullptr), R, "2^37 cells");
    expect(e2sar_hip_rows_advance(ctx, &wide, nullptr, 1, nullptr), R, "2^37 cells, advance");
    expect(e2sar_hip_rows_reassemble(nullptr, &good, pk, 64, ln, nullptr, 4, nullptr), P, "NULL ctx");
    expect(e2sar_hip_rows_reassemble(ctx, nullptr, pk, 64, ln, nullptr, 4, nullptr), P, "NULL descriptor");
    expect(e2sar_hip_rows_reassemble(ctx, &good, nullptr, 64, ln, nullptr, 4, nullptr), P, "NULL packets");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk, 64, nullptr, nullptr, 4, nullptr), P, "NULL lens");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk, 72, ln, nullptr, 4, nullptr), P, "stride not a multiple of 16");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk, 48, ln, nullptr, 4, nullptr), P, "stride too small");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk + 8, 64, ln, nullptr, 4, nullptr), P, "packets misaligned");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk, 64, ln, nullptr, (1u << 30) + 1u, nullptr), R, "batch too large");
    expect(e2sar_hip_rows_reassemble(ctx, &good, pk, 64, ln, nullptr, 0, nullptr), E2SAR_HIP_OK, "maxPackets 0");
    expect(e2sar_hip_rows_advance(nullptr, &good, nullptr, 1, nullptr), P, "advance, NULL ctx");
    expect(e2sar_hip_rows_advance(ctx, nullptr, nullptr, 1, nullptr), P, "advance, NULL descriptor");
    expect(e2sar_hip_rows_clear(nullptr, &good, 0, nullptr), P, "clear, NULL ctx");
    expect(e2sar_hip_rows_clear(ctx, nullptr, 0, nullptr), P, "clear, NULL descriptor");
    e2sar_hip_rows third = good;
    third.eventStep = 3;
    third.eventPhase = 2;
    expect(e2sar_hip_rows_clear(ctx, &third, 3, nullptr), P, "clear, eventBase off the lattice");
    expect(e2sar_hip_rows_clear(ctx, &third, ~0ull, nullptr), P, "clear, 2^64 - 1 is 0 mod 3");
    expect(e2sar_hip_rows_reassemble(ctx, &third, pk, 64, ln, nullptr, 0, nullptr), E2SAR_HIP_OK, "a lattice, maxPackets 0");
    std::printf("%s: %d failing\n", g_bad ? "FAILED" : "ok", g_bad);
    return g_bad ? 1 : 0;
}
