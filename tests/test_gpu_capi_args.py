"""The C ABI's argument checks: return code, exact message and the order the checks fire in.

Every expectation below is what the library returned before the launch prologue and the
argument checks of capi.cpp were gathered into shared helpers; a helper that reorders two
checks or rewords a message fails here.  No failing call reaches a kernel launch, and the
passing ones are empty batches, which return before one.
"""
import ctypes as C

import pytest
import torch

from e2sar_amd import _capi, sar
from e2sar_amd._capi import ERR_LOGIC, ERR_OUT_OF_RANGE, ERR_PARAMETER, E2SARHipError, check, lib

pytestmark = pytest.mark.gpu

P = ERR_PARAMETER
NULL = C.c_void_p(0)
HUGE = 0xFFFFFFFF            # nPackets * (stride / 16) above 2^32 for every legal stride
LOTS = 1 << 62               # a work buffer size no work_bytes() exceeds

STRIDE_16 = "stride must be a multiple of 16 and > header + 16"
ALIGN_16 = "packet buffer not 16-byte aligned"
WORK_256 = "work buffer not 256-byte aligned"
SEG_STRIDE = "stride must be a multiple of 16 and hold 36 + maxPldLen"
MAXPLD_0 = "maxPldLen is 0 (MTU too small)"
MAXPLD_BIG = "maxPldLen above a UDP datagram"
WORLD = "world must be 1..64, self < world"
ROUTE_STRIDE = "stride must be a multiple of 16, >= 48"


class Env:
    def __init__(self, ctx):
        self.ctx = ctx
        self.r = sar.DeviceReassembler(ctx, with_lb_header=True, table_slots=64, arena_bytes=1 << 20,
                                       compactable=True)
        self.plain = sar.DeviceReassembler(ctx, with_lb_header=False, table_slots=64, arena_bytes=1 << 20)
        self.buf = torch.zeros(1 << 16, dtype=torch.uint8, device=ctx.torch_device)
        base = (self.buf.data_ptr() + 255) & ~255
        self.pk = base                   # datagrams, 256-byte aligned
        self.ln = base + 0x4000          # lengths / counters
        self.wk = base + 0x8000          # work buffers
        self.wk2 = base + 0xA000
        self.out = base + 0xC000         # second datagram buffer
        self.need = lib().e2sar_hip_reas_work_bytes(4)


@pytest.fixture(scope="module")
def env(hip):
    e = Env(hip)
    yield e
    e.r.close()
    e.plain.close()


def p(addr):
    return C.c_void_p(addr)


def fails(code, msg, rc):
    with pytest.raises(E2SARHipError) as ei:
        check(rc)
    assert (ei.value.code, ei.value.msg) == (code, msg)


def test_reassemble_batch(env):
    f = lib().e2sar_hip_reassemble_batch
    r, pk, ln = env.r.handle, p(env.pk), p(env.ln)
    fails(P, "reas is NULL", f(NULL, pk, 64, ln, 4, 0, NULL))
    assert f(r, NULL, 0, NULL, 0, 0, NULL) == 0
    fails(P, "NULL device buffer", f(r, NULL, 64, ln, 4, 0, NULL))
    fails(P, "NULL device buffer", f(r, pk, 64, NULL, 4, 0, NULL))
    fails(P, STRIDE_16, f(r, pk, 72, ln, 4, 0, NULL))
    fails(P, STRIDE_16, f(r, pk, 48, ln, 4, 0, NULL))               # 36 + 16 = 52
    fails(P, STRIDE_16, f(env.plain.handle, pk, 32, ln, 4, 0, NULL))  # 20 + 16 = 36
    fails(P, ALIGN_16, f(r, p(env.pk + 8), 64, ln, 4, 0, NULL))
    fails(ERR_OUT_OF_RANGE, "batch too large", f(r, pk, 64, ln, HUGE, 0, NULL))
    # which message wins
    fails(P, "NULL device buffer", f(r, NULL, 72, ln, HUGE, 0, NULL))
    fails(P, STRIDE_16, f(r, p(env.pk + 8), 72, ln, HUGE, 0, NULL))
    fails(P, ALIGN_16, f(r, p(env.pk + 8), 64, ln, HUGE, 0, NULL))


def test_reas_classify(env):
    f = lib().e2sar_hip_reas_classify
    r, pk, ln, wk, need = env.r.handle, p(env.pk), p(env.ln), p(env.wk), env.need
    fails(P, "reas is NULL", f(NULL, pk, 64, ln, 4, 0, wk, need, NULL))
    assert f(r, NULL, 0, NULL, 0, 0, NULL, 0, NULL) == 0
    fails(P, "NULL device buffer", f(r, NULL, 64, ln, 4, 0, wk, need, NULL))
    fails(P, "NULL device buffer", f(r, pk, 64, NULL, 4, 0, wk, need, NULL))
    fails(P, "NULL device buffer", f(r, pk, 64, ln, 4, 0, NULL, need, NULL))
    fails(P, STRIDE_16, f(r, pk, 72, ln, 4, 0, wk, need, NULL))
    fails(P, STRIDE_16, f(r, pk, 48, ln, 4, 0, wk, need, NULL))
    fails(P, STRIDE_16, f(env.plain.handle, pk, 32, ln, 4, 0, wk, need, NULL))
    fails(P, ALIGN_16, f(r, p(env.pk + 8), 64, ln, 4, 0, wk, need, NULL))
    fails(ERR_OUT_OF_RANGE, "batch too large", f(r, pk, 64, ln, HUGE, 0, wk, LOTS, NULL))
    fails(P, WORK_256, f(r, pk, 64, ln, 4, 0, p(env.wk + 128), need, NULL))
    fails(P, "work buffer too small", f(r, pk, 64, ln, 4, 0, wk, need - 1, NULL))
    # which message wins: the work buffer is checked before the batch, alignment before size
    fails(P, WORK_256, f(r, p(env.pk + 8), 72, ln, 4, 0, p(env.wk + 128), need - 1, NULL))
    fails(P, "work buffer too small", f(r, p(env.pk + 8), 72, ln, HUGE, 0, wk, need, NULL))
    fails(P, "NULL device buffer", f(r, pk, 72, ln, 4, 0, NULL, 0, NULL))


def test_reas_scatter(env):
    f = lib().e2sar_hip_reas_scatter
    r, pk, wk, need = env.r.handle, p(env.pk), p(env.wk), env.need
    fails(P, "reas is NULL", f(NULL, pk, 64, 4, wk, need, NULL))
    assert f(r, NULL, 0, 0, NULL, 0, NULL) == 0
    fails(P, "NULL device buffer", f(r, NULL, 64, 4, wk, need, NULL))
    fails(P, "NULL device buffer", f(r, pk, 64, 4, NULL, need, NULL))
    fails(P, STRIDE_16, f(r, pk, 72, 4, wk, need, NULL))
    fails(P, STRIDE_16, f(r, pk, 48, 4, wk, need, NULL))
    fails(P, ALIGN_16, f(r, p(env.pk + 8), 64, 4, wk, need, NULL))
    fails(ERR_OUT_OF_RANGE, "batch too large", f(r, pk, 64, HUGE, wk, LOTS, NULL))
    fails(P, WORK_256, f(r, pk, 64, 4, p(env.wk + 128), need, NULL))
    fails(P, "work buffer too small", f(r, pk, 64, 4, wk, need - 1, NULL))
    fails(P, "work buffer too small", f(r, p(env.pk + 8), 72, 4, wk, 0, NULL))


def test_reas_scatter_classify(env):
    f = lib().e2sar_hip_reas_scatter_classify
    r, pk, ln, wk, wk2, need = env.r.handle, p(env.pk), p(env.ln), p(env.wk), p(env.wk2), env.need
    cpk = p(env.out)

    def call(r=r, stride=64, spk=pk, sn=4, swk=wk, sb=need, cpk=cpk, cln=ln, cn=4, cwk=wk2, cb=need):
        return f(r, stride, spk, sn, swk, sb, cpk, cln, cn, 0, cwk, cb, NULL)

    fails(P, "reas is NULL", call(r=NULL))
    assert call(spk=NULL, sn=0, swk=NULL, sb=0, cpk=NULL, cln=NULL, cn=0, cwk=NULL, cb=0) == 0
    fails(P, "NULL device buffer (scatter batch)", call(spk=NULL))
    fails(P, "NULL device buffer (scatter batch)", call(swk=NULL))
    fails(P, "NULL device buffer (classify batch)", call(cpk=NULL))
    fails(P, "NULL device buffer (classify batch)", call(cln=NULL))
    fails(P, "NULL device buffer (classify batch)", call(cwk=NULL))
    fails(P, STRIDE_16, call(stride=72))
    fails(P, STRIDE_16, call(stride=48))
    fails(P, STRIDE_16, call(stride=72, sn=0))
    fails(P, ALIGN_16, call(spk=p(env.pk + 8)))
    fails(P, ALIGN_16, call(cpk=p(env.out + 8)))
    fails(ERR_OUT_OF_RANGE, "batch too large", call(sn=HUGE, sb=LOTS))
    fails(ERR_OUT_OF_RANGE, "batch too large", call(cn=HUGE, cb=LOTS))
    fails(P, WORK_256, call(swk=p(env.wk + 128)))
    fails(P, WORK_256, call(cwk=p(env.wk2 + 128)))
    fails(P, "scatter work buffer too small", call(sb=need - 1))
    fails(P, "classify work buffer too small", call(cb=need - 1))
    fails(P, "the two batches need different work buffers", call(cwk=wk))
    # which message wins: the scatter batch is checked first, the shared buffer last
    fails(P, "scatter work buffer too small", call(sb=need - 1, cwk=NULL))
    fails(P, "NULL device buffer (classify batch)", call(swk=p(env.wk + 128), sn=0, cwk=NULL))
    fails(P, ALIGN_16, call(cpk=p(env.out + 8), cwk=wk))


def test_segment_entry_points(env):
    L = lib()
    ctx, r, ev, pk, ln = env.ctx.handle, env.r.handle, p(env.out), p(env.pk), p(env.ln)

    def batch(ctx=ctx, ev=ev, n=1, mp=100, pk=pk, stride=144):
        return L.e2sar_hip_segment_batch(ctx, ev, n, 1, 2, mp, 0, pk, stride, ln, NULL)

    def dev(ctx=ctx, ev=ev, n=1, mp=100, pk=pk, stride=144, counts=ln):
        return L.e2sar_hip_segment_batch_dev(ctx, ev, counts, n, 1, 2, mp, pk, stride, ln, NULL)

    def recycle(ctx=ctx, ev=ev, n=1, mp=100, pk=pk, stride=144, r=r):
        return L.e2sar_hip_segment_batch_recycle(ctx, ev, n, 1, 2, mp, 0, pk, stride, ln, r, 1, NULL)

    for f in (batch, dev, recycle):
        fails(P, "ctx is NULL", f(ctx=NULL))
        fails(P, "NULL device buffer", f(ev=NULL))
        fails(P, "NULL device buffer", f(pk=NULL))
        fails(P, MAXPLD_0, f(mp=0))
        fails(P, MAXPLD_BIG, f(mp=65536))
        fails(P, SEG_STRIDE, f(stride=152))
        fails(P, SEG_STRIDE, f(stride=128))                        # 36 + 100 = 136
        fails(P, ALIGN_16, f(pk=p(env.pk + 8)))
        # which message wins
        fails(P, MAXPLD_0, f(mp=0, stride=152, pk=p(env.pk + 8)))
        fails(P, SEG_STRIDE, f(stride=152, pk=p(env.pk + 8)))
    # an empty batch returns before the layout checks, except with a reassembler to recycle
    assert batch(ev=NULL, n=0, mp=0, pk=NULL, stride=0) == 0
    assert dev(ev=NULL, n=0, mp=0, pk=NULL, stride=0) == 0
    fails(P, MAXPLD_0, recycle(ev=NULL, n=0, mp=0, pk=NULL, stride=0))
    fails(P, "NULL device buffer", dev(counts=NULL))
    fails(P, "reas is NULL", recycle(r=NULL))
    fails(P, "ctx is NULL", recycle(ctx=NULL, r=NULL))
    if torch.cuda.device_count() >= 2:
        other = C.c_void_p()
        check(L.e2sar_hip_ctx_create(1, NULL, C.byref(other)))
        try:
            fails(P, "reassembler on another device", recycle(ctx=other))
            fails(P, "reassembler on another device", recycle(ctx=other, mp=0))
        finally:
            L.e2sar_hip_ctx_destroy(other)
            torch.cuda.set_device(0)


def test_route_entry_points(env):
    L = lib()
    ctx, pk, ln, out, wk = env.ctx.handle, p(env.pk), p(env.ln), p(env.out), p(env.wk)
    n = 300
    need = L.e2sar_hip_route_workspace_bytes(n, 2)
    assert need == 24

    def two_pass(fn):
        def call(ctx=ctx, stride=64, pk=pk, n=n, world=2, self_=0, ws=wk, wsb=need):
            return fn(ctx, pk, stride, ln, n, 1, world, self_, out, p(env.ln + 0x1000), p(env.ln + 0x2000), ws, wsb, NULL)
        return call

    def append(ctx=ctx, stride=64, pk=pk, n=n, world=2, self_=0, ws=wk, wsb=need, cap=16, running=ln):
        return L.e2sar_hip_route_append(ctx, pk, stride, ln, n, 1, world, self_, 0, out, p(env.ln + 0x1000), cap,
                                        running, ws, wsb, NULL)

    for f in (two_pass(L.e2sar_hip_route_batch), two_pass(L.e2sar_hip_route_foreign), append):
        fails(P, "ctx is NULL", f(ctx=NULL))
        fails(P, WORLD, f(world=0))
        fails(P, WORLD, f(world=65))
        fails(P, WORLD, f(world=2, self_=2))
        fails(P, ROUTE_STRIDE, f(stride=32))
        fails(P, ROUTE_STRIDE, f(stride=56))
        fails(P, "NULL device buffer", f(pk=NULL))
        fails(P, WORLD, f(world=0, stride=32, pk=NULL))
        fails(P, ROUTE_STRIDE, f(stride=32, pk=NULL))
    for fn in (L.e2sar_hip_route_batch, L.e2sar_hip_route_foreign):
        f = two_pass(fn)
        fails(P, "workspace too small", f(wsb=need - 1))
        fails(P, "NULL device buffer", f(ws=NULL, wsb=0))
    # the one-launch form takes no workspace: an empty batch with none passes
    assert append(n=0, ws=NULL, wsb=0) == 0
    fails(P, "capPerRank must be > 0 and capPerRank * world < 2^32", append(cap=0))
    fails(P, "capPerRank must be > 0 and capPerRank * world < 2^32", append(cap=0x80000000))
    fails(P, "NULL running counters", append(running=NULL))
    fails(P, "capPerRank must be > 0 and capPerRank * world < 2^32", append(cap=0, running=NULL, pk=NULL))
    fails(P, "NULL running counters", append(running=NULL, pk=NULL))


def test_reassembler_settings(env):
    L = lib()
    r = env.r.handle
    fails(P, "reas is NULL", L.e2sar_hip_reas_set_owner(NULL, 2, 0))
    fails(P, WORLD, L.e2sar_hip_reas_set_owner(r, 0, 0))
    fails(P, WORLD, L.e2sar_hip_reas_set_owner(r, 65, 0))
    fails(P, WORLD, L.e2sar_hip_reas_set_owner(r, 2, 2))
    fails(P, "reas is NULL", L.e2sar_hip_reas_compact(NULL, NULL))
    fails(ERR_LOGIC, "reassembler was not created COMPACTABLE", L.e2sar_hip_reas_compact(env.plain.handle, NULL))
    ev, cnt = p(env.out), p(env.ln)
    fails(P, "reas is NULL", L.e2sar_hip_relay_plan(NULL, 0, 4, 100, 0, 0, ev, cnt, NULL))
    fails(P, "NULL device buffer", L.e2sar_hip_relay_plan(r, 0, 4, 100, 0, 0, NULL, cnt, NULL))
    fails(P, "NULL device buffer", L.e2sar_hip_relay_plan(r, 0, 4, 100, 0, 0, ev, NULL, NULL))
    fails(P, "bad maxPldLen", L.e2sar_hip_relay_plan(r, 0, 4, 0, 0, 0, ev, cnt, NULL))
    fails(P, "bad maxPldLen", L.e2sar_hip_relay_plan(r, 0, 4, 65536, 0, 0, ev, cnt, NULL))
    fails(P, "NULL device buffer", L.e2sar_hip_relay_plan(r, 0, 4, 0, 0, 0, NULL, cnt, NULL))
    fails(P, "reas is NULL", L.e2sar_hip_reas_gc(NULL, 0, 0, NULL))
    fails(P, "reas is NULL", L.e2sar_hip_reas_recycle(NULL, 1, NULL))
    fails(P, "reas is NULL", L.e2sar_hip_reas_reset_stats(NULL, NULL))


@pytest.mark.skipif(not _capi.has_experimental(), reason="needs the experimental library (make experimental)")
def test_experimental_entry_points(env):
    L = lib()
    ctx, r, pk, ln, ev = env.ctx.handle, env.r.handle, p(env.pk), p(env.ln), p(env.out)
    g = L.e2sar_hip_reassemble_groups
    st = p(env.ln + 0x1000)
    fails(P, "reas is NULL", g(NULL, pk, 64, ln, 4, st, 1, 0, NULL))
    assert g(r, NULL, 0, NULL, 0, NULL, 0, 0, NULL) == 0
    fails(P, "NULL device buffer", g(r, NULL, 64, ln, 4, st, 1, 0, NULL))
    fails(P, STRIDE_16, g(r, pk, 72, ln, 4, st, 1, 0, NULL))
    fails(P, STRIDE_16, g(r, pk, 48, ln, 4, st, 1, 0, NULL))
    fails(P, ALIGN_16, g(r, p(env.pk + 8), 64, ln, 4, st, 1, 0, NULL))
    fails(ERR_OUT_OF_RANGE, "batch too large", g(r, pk, 64, ln, HUGE, st, 1, 0, NULL))
    fails(P, "too many groups", g(r, pk, 64, ln, 4, st, 0x80000000, 0, NULL))

    def chain(ctx=ctx, r=r, mp=100, stride=144, pk=pk, n=2):
        return L.e2sar_hip_segment_reassemble_batch(ctx, ev, 1, n, n, 2, mp, pk, stride, ln, r, 0, NULL)

    fails(P, "NULL argument", chain(ctx=NULL))
    fails(P, "NULL argument", chain(r=NULL))
    fails(P, MAXPLD_0, chain(mp=0))
    fails(P, MAXPLD_BIG, chain(mp=65536))
    fails(P, SEG_STRIDE, chain(stride=152))
    fails(P, SEG_STRIDE, chain(stride=128))
    fails(P, "the chained form emits LB headers: withLBHeader required", chain(r=env.plain.handle))
    fails(P, "NULL device buffer", chain(pk=NULL))
    fails(P, ALIGN_16, chain(pk=p(env.pk + 8)))
    fails(ERR_OUT_OF_RANGE, "batch too large", chain(n=HUGE))
    fails(P, SEG_STRIDE, chain(stride=152, pk=p(env.pk + 8), r=env.plain.handle))

    ng = C.c_uint32(7)
    one = (_capi.SegEvent * 1)()
    starts = (C.c_uint32 * 8)()
    s = L.e2sar_hip_seg_groups
    fails(P, "nGroups is NULL", s(one, 1, 1, 100, 144, starts, 8, None))
    fails(P, "NULL table", s(None, 1, 1, 100, 144, starts, 8, C.byref(ng)))
    assert ng.value == 0
    fails(P, MAXPLD_0, s(one, 1, 1, 0, 144, starts, 8, C.byref(ng)))
    fails(P, SEG_STRIDE, s(one, 1, 1, 100, 152, starts, 8, C.byref(ng)))
    fails(P, SEG_STRIDE, s(one, 1, 1, 100, 128, starts, 8, C.byref(ng)))
