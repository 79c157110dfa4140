"""The weight-gradient launch plan of csrc/ly_wgrad.hip, read back on the host through ly_wgrad_describe: the name of the contraction kernel
ly_wgrad / ly_wgrad_group would launch, formatted from the plan the launch itself consumes.  No GPU: the addresses below are made-up integers
with the alignment a case needs (ly_wgrad_describe dereferences none of them), the library is the built .so as in test_capi_abi.py.

The expected names are not taken from the code under test: the committed step's come from rocprofv3's own table of that step
(profiles/r07_train_bf16_step_kernels.txt), the branch cases' from the dispatch rules as DESIGN.md and the header state them."""
import collections
import ctypes
import os
import re

from lead_yolo_amd import capi, ops
from tests.test_gpu_wgrad1 import GEOM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DU, X, DW, WS, VEC = 0x10000000, 0x20000000, 0x30000000, 0x40000000, 0x50000000      # 16-byte aligned "device" addresses


def params(M, N, Cin, H=None, W=None, ks=1, stride=1, pad=0, Hin=None, Win=None, dtype=capi.LY_BF16, du=DU, x=X, ws=WS, lddu=None, nchw=0,
           pro=False):
    if H is None:
        _, H, W = GEOM[M]
    return capi.LyWgradParams(M=M, H=H, W=W, N=N, du=du, lddu=lddu or N, x=x, ldx=Cin, Hin=Hin or H, Win=Win or W, Cin=Cin, ks=ks, stride=stride,
                              pad=pad, nchw=nchw, up2=0, dw=DW, lddw=ks * ks * Cin, dtype=dtype, dw_ts=Cin, dw_cs=1, n_valid=N, c_valid=Cin,
                              x_scale=VEC if pro else None, x_shift=VEC + 4096 if pro else None, ws=ws, ws_floats=ops.WGRAD_WS_FLOATS if ws else 0)


def describe(*problems, cap=128):
    """(return code, name) of ly_wgrad_describe on the problems"""
    arr = (capi.LyWgradParams * len(problems))(*problems)
    name = ctypes.create_string_buffer(cap)
    rc = capi.lib().ly_wgrad_describe(arr, len(problems), name, cap)
    return rc, name.value.decode()


def test_the_committed_step_gets_the_names_rocprofv3_printed():
    """the 24 weight-gradient calls (38 problems) of the bs=64 bf16 step, profiles/r07_wgrad_shapes.txt, described one by one: the multiset of
    names is the launch count of every ly_wgrad* contraction row of that step's rocprofv3 table"""
    calls = []
    for line in open(os.path.join(ROOT, "profiles", "r07_wgrad_shapes.txt")):
        found = re.findall(r"M=\s*(\d+) N=\s*(\d+) K=\s*(\d+) (rows|k3s1|k2s2)", line)
        if not found:
            continue
        call = []
        for M, N, K, kind in ((int(m), int(n), int(k), kind) for m, n, k, kind in found):
            hw = {20 * 20 * 64: 20, 40 * 40 * 64: 40, 80 * 80 * 64: 80}[M]
            ks, stride, pad = {"rows": (1, 1, 0), "k3s1": (3, 1, 1), "k2s2": (2, 2, 0)}[kind]
            assert K % (ks * ks) == 0
            call.append(params(M, N, K // (ks * ks), H=hw, W=hw, ks=ks, stride=stride, pad=pad, Hin=hw * stride, Win=hw * stride))
        calls.append(call)
    assert len(calls) == 24 and sum(map(len, calls)) == 38
    got = collections.Counter()
    for call in calls:
        rc, name = describe(*call)
        assert rc == 0, (rc, name, capi.lib().ly_last_error())
        got[name] += 1

    table = collections.Counter()
    for line in open(os.path.join(ROOT, "profiles", "r07_train_bf16_step_kernels.txt")):
        m = re.match(r"(ly_wgrad\S*(?: \S+)*?)\s{2,}(\d+)\s+[\d.]+ us\s+[\d.]+ us\s*$", line)
        if m and "_combine" not in m[1]:
            table[m[1]] += int(m[2])
    by_hand = {"ly_wgrad1_group_kernel": 10, "ly_wgrad3_kernel": 5, "ly_wgrad1_kernel<32, 128, true>": 3, "ly_wgrad1_kernel<128, 128, true>": 2,
               "ly_wgrad_tiled_kernel<__bf16, 128, 128, 128, false, false, true>": 2,
               "ly_wgrad_tiled_kernel<__bf16, 64, 128, 128, false, false, true>": 1, "ly_wgrad1_kernel<64, 64, true>": 1}
    assert dict(table) == by_hand and sum(table.values()) == 24
    assert got == table


def _with(switch, value, fn):
    was = switch(value)
    try:
        return fn()
    finally:
        switch(was)


def test_every_branch_of_the_single_problem_plan():
    L = capi.lib()
    # the four tile classes; M = 1440 is three chunks of 512 pixels, so with scratch the slab form
    assert describe(params(1440, 64, 64)) == (0, "ly_wgrad1_kernel<64, 64, true>")
    assert describe(params(1440, 24, 128)) == (0, "ly_wgrad1_kernel<32, 128, true>")
    assert describe(params(1440, 40, 72)) == (0, "ly_wgrad1_kernel<64, 128, true>")
    assert describe(params(1440, 72, 200)) == (0, "ly_wgrad1_kernel<128, 128, true>")
    # ly_tune_wgrad1(0): the octet form of the register-transposing kernel for the same problem
    assert _with(L.ly_tune_wgrad1, 0, lambda: describe(params(1440, 24, 128))) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, false, true>")
    assert describe(params(1440, 24, 128)) == (0, "ly_wgrad1_kernel<32, 128, true>")
    # x on a quad but not on an octet boundary (8 bytes into a 16-byte vector) drops the octets: quad staging, and never wgrad1
    assert describe(params(1440, 24, 128, x=X + 8)) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, false, false>")
    assert describe(params(1440, 24, 128, du=DU + 8)) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, false, false>")
    # x two bytes off: not even whole quads, the per-lane gather kernel
    assert describe(params(1440, 24, 128, x=X + 2)) == (0, "ly_wgrad_kernel<__bf16, true>")
    # the x prologue: the PRO instantiation of the tiled kernel, never wgrad1
    assert describe(params(1440, 24, 128, pro=True)) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, true, true>")
    assert describe(params(64, 24, 128, pro=True)) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, true, true>")
    # no scratch: several chunks keep the atomic flush of the tiled kernel, one chunk adds straight from wgrad1
    assert describe(params(1440, 24, 128, ws=None)) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, true, false, true>")
    assert describe(params(64, 24, 128, ws=None)) == (0, "ly_wgrad1_kernel<32, 128, false>")
    assert describe(params(64, 24, 128)) == (0, "ly_wgrad1_kernel<32, 128, false>")             # one chunk needs no slab
    # fp32 storage: 64 pixels per step, quads
    assert describe(params(1440, 24, 128, dtype=capi.LY_F32)) == (0, "ly_wgrad_tiled_kernel<float, 32, 128, 64, true, false, false>")
    assert describe(params(1440, 72, 200, dtype=capi.LY_F32)) == (0, "ly_wgrad_tiled_kernel<float, 128, 128, 64, true, false, false>")
    # widths that are no whole quads, NCHW input: the generic kernel, rows / gather
    assert describe(params(1440, 6, 128)) == (0, "ly_wgrad_kernel<__bf16, true>")
    assert describe(params(1440, 24, 128, nchw=1)) == (0, "ly_wgrad_kernel<__bf16, false>")
    assert describe(params(1440, 6, 128, dtype=capi.LY_F32)) == (0, "ly_wgrad_kernel<float, true>")
    # 3x3 / stride 1 / pad 1 in bf16: the halo-tile kernel; with ly_tune_wgrad3(0) the gathered octet form of the tiled kernel
    k3 = dict(ks=3, stride=1, pad=1)
    assert describe(params(1440, 24, 128, **k3)) == (0, "ly_wgrad3_kernel")
    assert _with(L.ly_tune_wgrad3, 0, lambda: describe(params(1440, 24, 128, **k3))) == (0, "ly_wgrad_tiled_kernel<__bf16, 32, 128, 128, false, false, true>")
    assert describe(params(1440, 24, 128, dtype=capi.LY_F32, **k3)) == (0, "ly_wgrad_tiled_kernel<float, 32, 128, 64, false, false, false>")
    assert describe(params(1440, 24, 128, **k3)) == (0, "ly_wgrad3_kernel")


def test_every_branch_of_the_group_plan():
    L = capi.lib()
    a, b = params(1440, 72, 200), params(1440, 136, 8)
    assert describe(a, b) == (0, "ly_wgrad1_group_kernel")
    assert describe(a, b, params(960, 256, 136), params(480, 128, 128)) == (0, "ly_wgrad1_group_kernel")
    # without scratch: the grouped tiled kernel with the atomic flush (quads: the octets go with the slab form)
    assert describe(params(1440, 72, 200, ws=None), b) == (0, "ly_wgrad_tiled_group_kernel<__bf16, 128, 128, 128, true, false, false, false>")
    # both flush forms of the grouped tiled kernel, and what keeps a group off wgrad1: the switch, a prologue, a member without octets
    assert _with(L.ly_tune_wgrad1, 0, lambda: describe(a, b)) == (0, "ly_wgrad_tiled_group_kernel<__bf16, 128, 128, 128, true, false, true, true>")
    assert describe(a, params(1440, 136, 8, pro=True)) == (0, "ly_wgrad_tiled_group_kernel<__bf16, 128, 128, 128, true, true, true, true>")
    assert describe(a, params(1440, 76, 200, lddu=76)) == (0, "ly_wgrad_tiled_group_kernel<__bf16, 128, 128, 128, true, false, true, false>")
    f32 = [params(1440, 72, 200, dtype=capi.LY_F32), params(1440, 136, 8, dtype=capi.LY_F32)]
    assert describe(*f32) == (0, "ly_wgrad_tiled_group_kernel<float, 128, 128, 64, true, false, true, false>")
    # one member outside the 128 x 128 class (N = 64), mixed storage, more than four: n calls of ly_wgrad, return code 1
    assert describe(a, params(1440, 64, 128))[0] == 1
    assert describe(a, f32[1])[0] == 1
    assert describe(a, b, a, b, a)[0] == 1
    assert describe(a) == (0, "ly_wgrad1_kernel<128, 128, true>")


def test_refusals_carry_ly_wgrads_message():
    L = capi.lib()
    for bad, msg in [(params(1440, 24, 128, H=20, W=23), "wgrad: M is not a whole number of images"),
                     (params(1440, 24, 128, Hin=10), "wgrad: 1x1 gather needs Hin == H, Win == W"),
                     (params(1440, 6, 128, pro=True), "wgrad: the x prologue is built for plain-row 1x1 problems with vector-friendly widths"),
                     (params(1440, 24, 128, dtype=7), "wgrad")]:
        rc, _ = describe(bad)
        assert rc < 0 and msg in L.ly_last_error().decode(), (rc, L.ly_last_error())
        assert describe(params(1440, 72, 200), bad)[0] < 0                      # as a member of a group that falls back to single calls
    name = ctypes.create_string_buffer(16)
    one = (capi.LyWgradParams * 1)(params(1440, 24, 128))
    for args in [(None, 1, name, 16), (one, 0, name, 16), (one, 1, None, 16), (one, 1, name, 0)]:
        assert L.ly_wgrad_describe(*args) < 0 and "wgrad_describe: bad arguments" in L.ly_last_error().decode()


def test_describing_writes_nothing_but_the_name():
    L = capi.lib()
    full = "ly_wgrad_tiled_group_kernel<__bf16, 128, 128, 128, true, false, false, false>"
    arr = (capi.LyWgradParams * 2)(params(1440, 72, 200, ws=None), params(1440, 136, 8))
    before = bytes(arr)
    for cap in (128, len(full) + 1, len(full), 10, 1):
        buf = ctypes.create_string_buffer(b"\xaa" * (8 + cap + 8), 8 + cap + 8)
        assert L.ly_wgrad_describe(arr, 2, ctypes.byref(buf, 8), cap) == 0
        raw = bytes(buf)
        assert raw[:8] == b"\xaa" * 8 and raw[8 + cap:] == b"\xaa" * 8, f"cap={cap}: bytes outside name[cap] were written"
        want = full[:cap - 1].encode()
        assert raw[8:8 + len(want) + 1] == want + b"\0", f"cap={cap}: not the name cut to cap - 1 characters and terminated"
    assert bytes(arr) == before
