"""Micro-benchmark (GPU box): conv kernels on the headline shapes; sweeps wgrad split-K and epilogue options.
Modes: fwd | epi | wgrad | all (fwd and wgrad)."""
import ctypes as C, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "open-world-semantic-segmentation_amd")]
import torch
from dmlnet import _lib
from dmlnet._lib import ConvDesc, WgradDesc
lib = _lib.load()
st = torch.cuda.current_stream().cuda_stream
bf = torch.bfloat16

def timeit(fn, n=20):
    for _ in range(3): fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n): fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e-3

SHAPES = [  # B, H, W, C, N, k, dil
    (16, 48, 48, 256, 256, 3, 1), (16, 48, 48, 1024, 256, 1, 1), (16, 48, 48, 256, 1024, 1, 1),
    (16, 192, 192, 320, 256, 3, 1), (16, 48, 48, 2048, 256, 3, 12), (16, 192, 192, 64, 256, 1, 1),
    (16, 96, 96, 128, 512, 1, 1), (16, 48, 48, 512, 512, 3, 2)]
if os.environ.get("BENCH_SHAPES"):          # "B,H,W,C,N,k,d;..." overrides the list
    SHAPES = [tuple(int(v) for v in t.split(",")) for t in os.environ["BENCH_SHAPES"].split(";")]
which = sys.argv[1] if len(sys.argv) > 1 else "all"
for (B, H, W, Cc, N, k, dil) in SHAPES:
    pad = dil * (k // 2)
    x = torch.randn(B, H, W, Cc, device="cuda").to(bf)
    w = (torch.randn(N, k, k, Cc, device="cuda") * 0.05).to(bf)
    y = torch.empty(B, H, W, N, device="cuda", dtype=bf)
    dy = torch.randn(B, H, W, N, device="cuda").to(bf)
    M = B * H * W
    stats = torch.empty((M + 63) // 64 * N * 2, device="cuda")
    fl = 2.0 * M * N * k * k * Cc
    line = "B%d %dx%d C%d->N%d k%d d%d | " % (B, H, W, Cc, N, k, dil)
    if which in ("all", "fwd"):
        for use_stats in (True, False):
            d = ConvDesc(x=x.data_ptr(), w=w.data_ptr(), y=y.data_ptr(), bias=None, stats=stats.data_ptr() if use_stats else None,
                         B=B, Hi=H, Wi=W, C=Cc, ldx=Cc, Ho=H, Wo=W, N=N, ldy=N, R=k, S=k,
                         stride=1, dil=dil, pad=pad, dtype=1, y_f32=0, accum=0, mode=0)
            t = timeit(lambda: lib.dml_conv_igemm(C.byref(d), st))
            line += "fwd%s %.1fus %.0fTF | " % ("+st" if use_stats else "", t * 1e6, fl / t / 1e12)
            if use_stats:                                # the same with the K-split of the last round's tiles allowed
                tws = torch.empty(512 * 128 * 128, device="cuda"); tcnt = torch.zeros(128, dtype=torch.int32, device="cuda")
                d.tail_ws, d.tail_ws_elems, d.tail_counters, d.tail_counters_len = tws.data_ptr(), tws.numel(), tcnt.data_ptr(), 128
                t = timeit(lambda: lib.dml_conv_igemm(C.byref(d), st))
                line += "fwd+st+tail %.1fus %.0fTF | " % (t * 1e6, fl / t / 1e12)

    if which == "epi":
        # data gradient of this conv (output = B x H x W x Cc) with the fused epilogue options of the train step
        M_ = B * H * W
        wt = (torch.randn(Cc, k, k, N, device="cuda") * 0.05).to(bf)
        gx = torch.zeros(B, H, W, Cc, device="cuda", dtype=bf)
        rdz = torch.randn(B, H, W, Cc, device="cuda").to(bf)
        ypre = torch.randn(B, H, W, Cc, device="cuda").to(bf)
        mask = torch.randint(0, 256, (M_ * Cc // 8,), dtype=torch.uint8, device="cuda")
        mean, invstd = torch.randn(Cc, device="cuda") * 0.1, torch.rand(Cc, device="cuda") + 0.5
        part = torch.empty((M_ + 63) // 64 * Cc * 2, device="cuda")
        tws = torch.empty(512 * 128 * 128, device="cuda"); tcnt = torch.zeros(128, dtype=torch.int32, device="cuda")
        fl_ = 2.0 * M_ * N * k * k * Cc
        for nm, acc_, res_, bnr_ in (("plain", 0, 0, 0), ("accum", 1, 0, 0), ("res", 0, 1, 0), ("bnr", 0, 0, 1), ("res+bnr", 0, 1, 1)):
            d = ConvDesc(x=dy.data_ptr(), w=wt.data_ptr(), y=gx.data_ptr(), bias=None, stats=None, B=B, Hi=H, Wi=W, C=N, ldx=N, Ho=H, Wo=W, N=Cc, ldy=Cc, R=k, S=k, stride=1, dil=dil, pad=pad, dtype=1,
                         y_f32=0, accum=acc_, mode=1)
            d.tail_ws, d.tail_ws_elems, d.tail_counters, d.tail_counters_len = tws.data_ptr(), tws.numel(), tcnt.data_ptr(), 128
            if res_:
                d.res_dz, d.res_mask, d.res_ld = rdz.data_ptr(), mask.data_ptr(), Cc
            if bnr_:
                d.bnr_y, d.bnr_mask, d.bnr_mean, d.bnr_invstd = ypre.data_ptr(), mask.data_ptr(), mean.data_ptr(), invstd.data_ptr()
                d.bnr_partials, d.bnr_ldy, d.bnr_relu = part.data_ptr(), Cc, 1
            t = timeit(lambda: lib.dml_conv_igemm(C.byref(d), st))
            by = 2.0 * M_ * (N + Cc * (1 + acc_ + res_ + bnr_)) + M_ * Cc / 8 * (res_ + bnr_)
            line += "%s %.1fus %.0fTF %.2fTB/s | " % (nm, t * 1e6, fl_ / t / 1e12, by / t / 1e12)
    if which in ("all", "wgrad"):
        dw = torch.zeros(N, k, k, Cc, device="cuda")
        for sk in (0, 4, 8, 16, 32, 64):
            wg = WgradDesc(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(), B=B, Hi=H, Wi=W, C=Cc, ldx=Cc, Ho=H, Wo=W, N=N,
                           ldy=N, R=k, S=k, stride=1, dil=dil, pad=pad, dtype=1, splitk=sk)
            t = timeit(lambda: lib.dml_conv_wgrad(C.byref(wg), st))
            line += "wg sk%d %.1fus %.0fTF | " % (sk, t * 1e6, fl / t / 1e12)
        ws = torch.empty(40 << 20, device="cuda")
        for sk in (0, 8, 16, 32, 64):
            wg = WgradDesc(x=x.data_ptr(), dy=dy.data_ptr(), dw=dw.data_ptr(), B=B, Hi=H, Wi=W, C=Cc, ldx=Cc, Ho=H, Wo=W, N=N,
                           ldy=N, R=k, S=k, stride=1, dil=dil, pad=pad, dtype=1, splitk=sk, Cm=0, ws=ws.data_ptr(),
                           ws_elems=ws.numel())
            t = timeit(lambda: lib.dml_conv_wgrad(C.byref(wg), st))
            line += "WS sk%d %.1fus %.0fTF | " % (sk, t * 1e6, fl / t / 1e12)
    print(line)
