"""GPU: the forward and data-gradient kernels behind dml_conv_igemm at their tile edges, through the C ABI -- every case of
tests/conv_cases.py: the register-staged conv_igemm_kernel, the LDS-DMA ring conv_igemm_dma_kernel, the three-term conv_igemm_x3_kernel
and the persistent conv_ws_kernel in its bf16 and two-plane forms with the four data-gradient epilogue instantiations.

Per case, kind of input and placement, one launch with x, y and every epilogue operand as channel slices of wider buffers (first / last
channel offset, NaN in the neighbouring channels of the inputs, the 0xAA sentinel in y's neighbours, in the whole old y where the launch
does not accumulate, and around every buffer), the fp16 planes written by dml_h2_split (layout 0 on the slice, layout 1 for the weights):
  exact inputs   an fp32 y must EQUAL the float64 result, a bf16 y its one round-to-nearest-even bf16 value; the sum half of stats and both
                 halves of bnr_partials are equal too (tests/conv_cases.py has the argument, tests/test_conv_refs.py proves it and proves that
                 every case reaches the kernel, grid, tiling, tail split and statistics rows its row claims);
  real inputs    |y - float64| <= (c 2^-24 + r) (sum |x w| + |extras|) per element, for a bf16 y plus half a bf16 spacing of its binade
                 (up to 2^-8 |y|: bf16's unit roundoff); the statistics and BatchNorm-backward partials inside their derived bars, per
                 group and merged by dml_bn_finalize / dml_bn_bwd_finalize;
  every sentinel byte and every input byte unchanged, no NaN in any output; a refused descriptor returns its code and writes nothing;
  the K-split tail runs twice with bitwise equal results, zeroed counters, and equals the unsplit launch bitwise on the exact inputs;
  the bf16 persistent kernel equals the ring kernel bitwise (ws_min_tiles = INT32_MAX on the same descriptor).
Each float check prints "MEASURE <what> err=<error at the largest share of its bar> bar=<that bar>" before it asserts (-s shows them).

Measured on the MI355X: the whole file, 181 tests, takes about 20 s (the slowest test, ws_dg_wrap144 with its float64 references and the
ring-kernel rerun, 1.7 s; the float64 references of the 256-row-tile cases about 1 s each).  Every exact case equals float64 bit for bit in
every family -- the second tile of a persistent workgroup, the K-split tail, both second-split-term cases (x3_mid, pl_fwd_h2_lo), all four
epilogue instantiations of the two-plane data gradient and the four parity classes assembled -- every sentinel and NaN neighbour is intact,
the bf16 persistent kernel equals the ring kernel bitwise.  No kernel and no rule of csrc/conv_choice.h had to be changed.
Largest measured share of the bar on real inputs (error of bar):
    y, fp32 out   conv_igemm_kernel<f32>  0.028 (2.3e-6 of 8.2e-5, f32_c12_n136_dg, c = 128)   conv_igemm_x3_kernel  0.047 (5.2e-7 of 1.1e-5, c = 32)
                  two-plane conv_ws_kernel 0.116 (1.9e-6 of 1.6e-5, pl_fwd_wrap144, c = 32)     bf16 operands, y_f32  0.003 (reg_bf16_c40_n64)
    y, bf16 out   0.95 - 0.999 in every family: the bar there is the half bf16 spacing of the one final rounding, which ties reach and
                  nothing passes (1.56e-2 of 1.56e-2 at |y| in [4, 8)); what lies below it is pinned by the exact inputs
    stats         sum 0.050 (m49_tile48), M2 0.010 (pl_fwd_wrap48); merged mean 0.005, merged 1 / sigma 0.007
    bnr_partials  0.09 / 0.16 (ws_dg_wrap144: sums of bf16-rounded g); merged 0.004;  assembled parity classes 0.015
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers as H  # noqa: F401  (path setup)
import conv_cases as CC
from test_gpu_pool_resize_edges import DT, Buf, check_le, chk, st
from test_gpu_wgrad_edges import Operand, Planes

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
PLACES = ("first", "last")
KINDS = ("exact", "real")
RUN = [c for c in CC.CASES if c.rc == 0]
BN_EPS = 1e-5
_REF = {}


@pytest.fixture(scope="module")
def lib():
    from dmlnet import _lib
    return _lib.load()


def reference(case, kind, inp=None):
    """(inputs, float64 reference, bar of y) of a case, computed once per module and shared"""
    key = (case.id, kind)
    if key not in _REF:
        inp = CC.inputs(case, kind) if inp is None else inp
        ref = CC.reference(case, inp)
        _REF[key] = (inp, ref, CC.y_bar(case, inp, ref) if kind == "real" else None)
        for d in (inp, ref):
            for a in d.values():
                a.setflags(write=False)
    return _REF[key]


def dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


class Job:
    """the device side of one launch: operands, planes, y and its descriptor"""

    def __init__(self, lib, case, kind, place, inp=None):
        from dmlnet._lib import ConvDesc, PrepDesc
        self.lib, self.case, self.kind = lib, case, kind
        self.inp, self.ref, self.bar = reference(case, kind, inp)
        c, inp, e = case, self.inp, case.epi
        ox, oy = c.offsets(place)
        self.oy = oy
        self.xo = Operand(c.Mx, c.C, c.ldx, ox, c.dtype, inp["x"])
        self.keep = [self.xo]
        wm = dev(inp["w"].reshape(c.N, c.Ktot))
        if c.ws:
            self.w = torch.empty(c.N * c.Ktot, device="cuda", dtype=torch.bfloat16)
            arr = (PrepDesc * 1)(PrepDesc(wm.data_ptr(), self.w.data_ptr(), None, c.N, c.R * c.S, c.C, c.C, 1, 0))
            tab = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
            chk(lib.dml_prep_weights(tab.data_ptr(), 1, 1, st()))
        else:
            self.w = wm.to(DT[c.dtype][1])
        self.wsnap = self.w.clone()
        self.d = d = ConvDesc(x=self.xo.ptr, w=self.w.data_ptr(), y=None, bias=None, stats=None, B=c.B, Hi=c.Hi, Wi=c.Wi, C=c.C, ldx=c.ldx,
                              Ho=c.Ho, Wo=c.Wo, N=c.N, ldy=c.ldy, R=c.R, S=c.S, stride=c.stride, dil=c.dil, pad=c.pad, dtype=DT[c.dtype][0],
                              y_f32=int("y_f32" in e), accum=int("accum" in e), mode=c.mode)
        d.f32_split = {"bf16": 0, "f32": 0, "x3": 1, "planes": 2}[c.kind]
        if c.ws:
            d.w_tiled, d.ws_min_tiles = 1, 1
        if c.kind == "planes":
            xp = Planes(lib, self.xo, c.Mx, c.C, c.ldx, ox)
            self.wplanes = torch.empty((2, c.N * c.Ktot), device="cuda", dtype=torch.float16)
            self.wwork = torch.zeros(1025, device="cuda")
            lay = 1 if (c.N % 64 == 0 and c.Ktot % 32 == 0) else 0
            chk(lib.dml_h2_split(wm.data_ptr(), c.N, c.Ktot, c.Ktot, self.wplanes.data_ptr(), c.N * c.Ktot, c.Ktot, lay, self.wwork.data_ptr(), 0, st()))
            if kind == "exact":
                assert xp.work[1024].item() == 2.0 ** -13 == self.wwork[1024].item()
                lo = xp.buf.region()[c.Mx:].view(torch.int16)
                assert bool(lo.any()) == (c.special == "h2_lo") == bool(self.wplanes[1].view(torch.int16).any())
            d.x_planes, d.x_unscale, d.x_plane_stride = xp.ptr, xp.unscale, xp.stride
            d.w_planes, d.w_unscale, d.w_plane_stride = self.wplanes.data_ptr(), self.wwork.data_ptr() + 4096, c.N * c.Ktot
            assert xp.stride == c.Mx * c.ldx
            self.keep.append(xp)
            if c.planes_only:
                d.x = xp.ptr
        if c.sub is not None:
            d.sub_grid, d.sub_y, d.sub_x = 1, c.sub[0], c.sub[1]
        if c.pad_w_set:
            d.pad_w_set, d.pad_w = 1, c.pad_x
        self.vecs = {}

        def vec(name):
            self.vecs[name] = dev(inp[name])
            return self.vecs[name].data_ptr()

        def side(name, dtype):
            o = Operand(c.My, c.N, c.ldy, oy, dtype, inp[name])
            self.keep.append(o)
            return o.ptr

        def mask(name):
            self.vecs[name] = dev(CC.pack_mask(inp[name], c.vec), torch.uint8)
            return self.vecs[name].data_ptr()
        if "bias" in e:
            d.bias = vec("bias")
        if "post" in e:
            d.post_scale, d.post_shift, d.post_mean, d.post_relu = vec("post_scale"), vec("post_shift"), vec("post_mean"), int("post_relu" in e)
            if "post_res" in e:
                d.post_res, d.post_ldres = side("res", c.dtype), c.ldy
        if "acc32" in e:
            d.acc32, d.acc32_ld = side("acc32", "f32"), c.ldy
        if "res" in e:
            d.res_dz, d.res_mask, d.res_ld = side("res", c.dtype), mask("res_on"), c.ldy
        if "bnr" in e:
            d.bnr_y, d.bnr_mean, d.bnr_invstd, d.bnr_ldy = side("bnr_y", c.dtype), vec("bnr_mean"), vec("bnr_invstd"), c.ldy
            d.bnr_relu, d.bnr_inc = int("bnr_relu" in e), int("bnr_inc" in e)
            if "bnr_relu" in e:
                d.bnr_mask = mask("bnr_on")
        self.rows = lib.dml_conv_stat_rows(C.byref(d))
        self.G = -(-c.M // self.rows)
        self.fresh()

    def fresh(self):
        """a new y (the sentinel, or the old value of an accumulating launch) and new partial buffers"""
        c, d = self.case, self.d
        self.y = Buf(c.My, c.N, c.ldy, self.oy, c.out_dtype, data=self.inp["old"] if "accum" in c.epi else None)
        d.y = self.y.ptr
        self.y0 = self.y.raw.clone()
        self.stats = self.part = None
        if "stats" in c.epi:
            self.stats = Buf(1, self.G * c.N * 2, dtype="f32")
            self.stats.region().fill_(float("nan"))               # (an unwritten partial stays NaN: the sentinel is a finite float)
            d.stats = self.stats.ptr
        if "bnr" in c.epi:
            self.part = Buf(1, self.G * c.N * 2, dtype="f32")
            self.part.region().fill_(float("nan"))
            d.bnr_partials = self.part.ptr

    def launch(self):
        return self.lib.dml_conv_igemm(C.byref(self.d), st())

    def intact(self):
        for o in self.keep:
            o.intact()
        assert torch.equal(self.w, self.wsnap), "the weights were written"

    def check(self, what):
        """y against the float64 result (equal, or inside the bar), the partials, the sentinels, the inputs; returns y's bits"""
        c = self.case
        rows = CC.out_rows(c)
        got = self.y.get().astype(F64)[rows]
        assert np.isfinite(got).all(), what + ": y is not finite"
        if self.kind == "exact":
            bad = got != self.ref["stored"]
            assert not bad.any(), "%s: %d of %d elements differ from the exact value, the first at %s (%r, expected %r)" % (
                what, int(bad.sum()), bad.size, np.argwhere(bad)[0].tolist(), got[bad][0], self.ref["stored"][bad][0])
        else:
            check_le("conv %s %s c=%d" % (c.kernel, what, CC.conv_chain(c)), np.abs(got - self.ref["y"]), self.bar)
        if c.sub is None:
            self.y.untouched()
        else:                       # the other three parity classes' pixels, the neighbouring channels and the guards
            now = self.y.raw.clone()
            keep = torch.ones(c.My, dtype=torch.bool)
            keep[torch.from_numpy(rows)] = False
            esz = self.y.esize
            body0 = self.y0[-(self.y.rows * self.y.ld + 256) * esz:-256 * esz].view(c.My, -1)
            body1 = now[-(self.y.rows * self.y.ld + 256) * esz:-256 * esz].view(c.My, -1)
            assert torch.equal(body0[keep.cuda()], body1[keep.cuda()]), what + ": a pixel of another parity class was written"
            lo, hi = self.oy * esz, (self.oy + c.N) * esz
            assert torch.equal(body0[:, :lo], body1[:, :lo]) and torch.equal(body0[:, hi:], body1[:, hi:])
        for name, buf in (("stats", self.stats), ("bnr", self.part)):
            if buf is None:
                continue
            p = buf.get().reshape(self.G, c.N, 2).astype(F64)
            assert np.isfinite(p).all(), "%s: %s partials unwritten (the NaN prefill) or not finite" % (what, name)
            buf.untouched()
            want = self.ref[name]
            if self.kind == "exact":
                halves = (0,) if name == "stats" else (0, 1)
                for h in halves:
                    assert (p[..., h] == want[..., h]).all(), "%s: %s partials, half %d, differ from the exact sums" % (what, name, h)
            bars = (CC.stats_bars if name == "stats" else CC.bnr_bars)(c, self.inp, self.ref)
            for h in (0, 1):
                check_le("%s half %d %s %s" % (name, h, c.kernel, what), np.abs(p[..., h] - want[..., h]), bars[..., h])
            self.merged(name, buf, p, want, bars, what)
        self.intact()
        return self.y.bits()

    def merged(self, name, buf, p, want, bars, what):
        """the partials merged by the library's finalize kernels against float64 statistics of the float64 convolution"""
        c, lib = self.case, self.lib
        conv = self.ref["conv"]
        if name == "stats":
            sc, sh, mu, inv = (torch.empty(c.N, device="cuda") for _ in range(4))
            chk(lib.dml_bn_finalize(buf.ptr, c.M, c.N, self.rows, None, None, None, None, 0.1, BN_EPS, sc.data_ptr(), sh.data_ptr(), mu.data_ptr(),
                                    inv.data_ptr(), st()))
            mean, var = conv.mean(0), conv.var(0)
            # mean = (sum of the G group sums) / M: the groups' own bars, G + 2 more fp32 roundings of the total
            mean_bar = (bars[..., 0].sum(0) + (self.G + 2) * CC.EPS32 * np.abs(want[..., 0]).sum(0)) / c.M
            check_le("merged mean %s" % what, np.abs(mu.cpu().numpy().astype(F64) - mean), mean_bar)
            # var = (sum M2_g + sum cnt_g (mean_g - mean)^2) / M: every term is positive, G + 8 roundings of the total; the group means
            # carry em_g = bar of the group's sum / cnt_g, the mean mean_bar
            g, ok = CC.groups(c, conv, self.rows)
            cnt = ok.sum(1)[:, None].astype(F64)
            dm = np.abs(g.sum(1) / cnt - mean)
            em = bars[..., 0] / cnt + mean_bar
            var_bar = (bars[..., 1].sum(0) + (cnt * (2 * dm * em + em * em)).sum(0)) / c.M + (self.G + 8) * CC.EPS32 * var
            istd = (var + BN_EPS) ** -0.5
            check_le("merged 1/sigma %s" % what, np.abs(inv.cpu().numpy().astype(F64) - istd), 0.5 * istd ** 3 * var_bar + 4 * CC.EPS32 * istd)
        else:
            ones = torch.ones(c.N, device="cuda")
            dg, db, coef = torch.zeros(c.N, device="cuda"), torch.zeros(c.N, device="cuda"), torch.empty(4 * c.N, device="cuda")
            chk(lib.dml_bn_bwd_finalize(buf.ptr, self.G, c.M, c.N, ones.data_ptr(), self.vecs["bnr_mean"].data_ptr(),
                                        self.vecs["bnr_invstd"].data_ptr(), dg.data_ptr(), db.data_ptr(), coef.data_ptr(), st()))
            for h, t in ((0, db), (1, dg)):
                bar = bars[..., h].sum(0) + (self.G + 2) * CC.EPS32 * np.abs(want[..., h]).sum(0)
                check_le("merged bnr sums half %d %s" % (h, what), np.abs(t.cpu().numpy().astype(F64) - want[..., h].sum(0)), bar)


# ---------------------------------------------------------------------------------------------------------------------
# one launch per case, kind and placement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("case", [c for c in RUN if not c.tail], ids=lambda c: c.id)
def test_conv_case(lib, case, place):
    for kind in KINDS:
        if case.special and kind == "real":
            continue                    # (the special cases differ from their base case on the exact inputs only)
        job = Job(lib, case, kind, place)
        assert job.rows == case.stat_rows
        chk(job.launch())
        bits = job.check("%s %s %s" % (case.id, kind, place))
        if case.ws:                     # the same descriptor on the ring kernel: same products in the same K order
            job.fresh()
            job.d.ws_min_tiles = CC.INT32_MAX
            assert lib.dml_conv_stat_rows(C.byref(job.d)) == 64
            job.stats = job.part = None
            G64 = -(-case.M // 64)
            scratch = torch.zeros(G64 * case.N * 2, device="cuda")
            if "stats" in case.epi:
                job.d.stats = scratch.data_ptr()
            if "bnr" in case.epi:
                job.d.bnr_partials = scratch.data_ptr()
            chk(job.launch())
            ring = job.y.bits()
            assert (ring == bits).all(), "%s: %d elements differ from the ring kernel's" % (case.id, int((ring != bits).sum()))
            job.y.untouched()


@pytest.mark.parametrize("place", PLACES)
@pytest.mark.parametrize("case", [c for c in RUN if c.tail], ids=lambda c: c.id)
def test_conv_tail_case(lib, case, place):
    """the K-split tail: twice in a row with bitwise equal results and zeroed counters; on the exact inputs bitwise the unsplit launch"""
    assert case.tail_q > 1
    ws = torch.full((CC.TAIL_WS_ELEMS,), float("nan"), device="cuda")
    cnt = torch.zeros(CC.TAIL_COUNTERS, dtype=torch.int32, device="cuda")
    for kind in KINDS:
        job = Job(lib, case, kind, place)
        d = job.d
        outs = []
        for run in range(2):
            if run:
                job.fresh()
            d.tail_ws, d.tail_ws_elems, d.tail_counters, d.tail_counters_len = ws.data_ptr(), ws.numel(), cnt.data_ptr(), cnt.numel()
            chk(job.launch())
            assert int(cnt.abs().sum()) == 0, "tail_counters are not zero after the launch"
            outs.append(job.check("%s %s %s run %d" % (case.id, kind, place, run)))
        assert (outs[0] == outs[1]).all(), "%s: the second launch differs at %d elements" % (case.id, int((outs[0] != outs[1]).sum()))
        assert not bool(torch.isnan(ws[:8 * case.tail_q * 128 * 128]).any()), "the tail workspace was not used"
        if kind == "exact":
            job.fresh()
            d.tail_ws, d.tail_ws_elems, d.tail_counters, d.tail_counters_len = None, 0, None, 0
            chk(job.launch())
            plain = job.check("%s exact unsplit" % case.id)
            assert (plain == outs[0]).all(), "%s: differs from the unsplit launch" % case.id


def test_refused_descriptor_writes_nothing(lib):
    """Ktot = 32 in a two-plane data gradient with the activation as planes only (x == x_planes): DML_EUNSUPPORTED, y untouched; the same
    descriptor with an fp32 tensor behind x runs the three-term kernel (pl_dg_k32_falls_to_x3, in test_conv_case)"""
    case = CC.BY_ID["pl_dg_k32_planes_only"]
    for place in PLACES:
        job = Job(lib, case, "exact", place)
        assert job.d.x == job.d.x_planes
        assert job.launch() == CC.EUNSUPPORTED
        torch.cuda.synchronize()
        assert torch.equal(job.y.raw, job.y0), "a refused launch wrote to y"
        job.intact()


# ---------------------------------------------------------------------------------------------------------------------
# the parity classes of a stride-2 data gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("place", PLACES)
def test_parity_classes_assemble_the_stride2_gradient(lib, place):
    """each class launch alone (its pixels against its own reference, the other classes' pixels bitwise unchanged), then the four into one
    tensor: the 3 x 3 stride-2 data gradient plus the value y held -- equal on the exact inputs, inside the classes' bars on the real ones"""
    p = CC.SUB_PARENT
    for kind in KINDS:
        pin = CC.inputs(p, kind)
        want = CC.reference(p, pin)["y"]
        jobs = []
        for c, rs, ss in CC.parity_classes():
            inp = dict(pin)
            inp["w"] = np.ascontiguousarray(pin["w"][:, rs][:, :, ss])
            _REF.pop((c.id, kind), None)
            job = Job(lib, c, kind, place, inp=inp)
            assert job.rows == 48
            chk(job.launch())
            job.check("%s %s %s" % (c.id, kind, place))
            jobs.append(job)
        first = jobs[0]
        first.fresh()
        for job in jobs:
            job.d.y = first.y.ptr
            chk(job.launch())
        got = first.y.get().astype(F64)
        first.y.untouched()
        if kind == "exact":
            assert (got == want).all(), "%d elements of the assembled gradient differ" % int((got != want).sum())
        else:
            bar = np.zeros_like(want)
            for job in jobs:
                bar[CC.out_rows(job.case)] = job.bar
            check_le("assembled stride-2 gradient %s" % place, np.abs(got - want), bar)
