"""Case table shared by tests/test_wgrad_refs.py (CPU) and tests/test_gpu_wgrad_edges.py (GPU): the weight gradient of
include/dmlnet_hip.h (dml_conv_wgrad, dml_conv_wgrad_group) as a plain numpy definition, the seeded inputs, the error bars and the
cases.  A plain module (no fixtures, no hooks, numpy only); nothing here looks at a kernel's output or imports the library.

The contract, in float64:
    dw[n][r][s][c] = dw0[n][r][s][c] + sum over (b, yo, xo) of dy[b][yo][xo][n] * x[b][yo stride - pad + r dil][xo stride - pad + s dil][c]
with 0 outside the image and only c < Cm kept -- written with np.pad, strided slices and tensordot (wgrad_ref), never with a kernel's
index arithmetic.

Two kinds of input.
  exact  x and dy integers in [-3, 3], dw beforehand integers in [-8, 8].  Every product is an integer of magnitude at most 9 and every
         partial sum of at most M <= 18432 of them, plus the value dw held, an integer below 9 * 18432 + 8 < 2^24: float32 holds
         every one of them, so ANY order of float32 additions is exact -- inside a workgroup's accumulators, across the fp32
         atomics, through the workspace slabs and both fold launches.  The operands are exact in every format the kernels read them
         in: bfloat16 holds the integers up to 256; the three-term bfloat16 split of such a value is hi = x, mid = lo = 0
         (x3_terms); dml_h2_split scales by the power of two s that puts max |x| = 3 into [2^14, 2^15), s = 2^13, and 3 * 2^13 has two
         significant bits, so hi = s x, lo = 0 (h2_terms), and the result is unscaled by the exact power of two 1 / (s_x s_dy), which
         moves an integer below 2^24 times 2^26 back without rounding.  Every family must therefore EQUAL the float64 result.
         One X3 case (x3_mid_terms, M = 25) has exact inputs of another make, because integers leave the split's cross products
         untested: x = a + b 2^-8 with a in {+-2, +-3} and b = +-1.  bfloat16 has a spacing of 2^-6 in [2, 4), so hi = a, mid = b 2^-8,
         lo = 0; the kept products hi hi, hi mid, mid hi, mid mid are multiples of 2^-16 and every partial sum is one below
         25 * (3 + 2^-8)^2 + 8 < 2^8 = 2^24 * 2^-16: exact again in any order, and wrong by at least 2^-16 if a product is missing.
  real   seeded Gaussians (rounded to bfloat16 for the bf16 cases); one case per family ("scaled") multiplies the activations by 1e3
         and the gradients by 1e-4, as test_conv_f16_two_plane_split_is_fp32_accurate does.  Per element of dw the bar is
             (c * 2^-24 + r) * (|dw0| + sum |dy * x|).
         c = wgrad_chain(case) is the any-order summation bound, counted from the code: a workgroup sums the 32 * slab_tiles pixel
         rows of its slab (32 per K step, rows past M are zeros and are counted), the fold (or the atomics) then adds the splitk
         slabs -- in chunks of 16 and then the chunk sums when the fold takes two launches, which changes the order and not the
         number of terms -- and the value dw held is one more term.  The products themselves are exact in the float32
         accumulator for every narrow format (bfloat16 x bfloat16 has 16 significant bits, fp16 x fp16 has 22) and the fp32
         MFMA fuses its product.
         r is the part of the error that is not summation:
           PLAIN, N64, BIG (bf16 operands as stored) and PLAIN float32 (f32_split = 0, the exact MFMA)    r = 0
           X3 (f32_split = 1; the header: "x = hi + mid + lo, six bf16 MFMAs per block").  bfloat16 keeps 8 significant bits, so
             |mid| <= 2^-8 |x| and |lo| <= 2^-16 |x|, and hi + mid + lo = x exactly: x - hi has at most 16 significant bits and is
             a float32, mid takes its upper 8, lo the rest (test_wgrad_refs.py checks this on the inputs used; residuals below
             2^-126 are flushed, which seeded Gaussians do not reach).  Of the nine products the kernel keeps six -- hi hi, hi mid,
             mid hi, hi lo, lo hi, mid mid -- and drops mid lo, lo mid (each <= 2^-24 |dy x|) and lo lo (<= 2^-32 |dy x|):
                                                                                                            r = 2 * 2^-24 + 2^-32
           H2 and WS (f32_split = 2 with planes; the header: "x s = xh + xl ... per block wl xh + wh xl + wh xh").  fp16 keeps 11
             significant bits: |xl| <= 2^-11 |s x| and the rounding of xl leaves |s x - xh - xl| <= 2^-22 |s x| (dml_h2_split's own
             "s x = hi + lo up to 2^-22 relative"), the same for dy: the two representation errors enter the product once each,
             2^-22 + 2^-22 (+ their product, 2^-44), and the dropped cross term dyl xl is at most 2^-11 * 2^-11 = 2^-22 of |dy x|:
                                                                                                            r = 3 * 2^-22 + 2^-44
             (An element below about 2^-17 of its tensor's largest has a lo plane in fp16's subnormal range, spacing 2^-24: its
             representation error is bounded by 2^-25 / s <= 2^-39 of the largest element instead of 2^-22 of itself.  A handful
             of the Gaussians used are that small; test_wgrad_refs.py emulates the split of the very inputs and asserts, per element
             of dw, that the representation errors they actually carry sum to less than the 2 * 2^-22 share r gives them.)
         No bar is measured on a kernel.  The GPU file prints the measured share of the bar.

Buffers (built by the GPU file from what this module describes): x and dy are channel slices [.., off : off + C] of wider buffers
with pitch ldx / ldy, at offset 0 ("first") or at the last offset ld - C ("last": the slice's last row ends with the allocation),
the neighbouring channels hold NaN; the fp16 planes come from dml_h2_split on the slice with ldp = ld.

The case table: every row gives B, Hi, Wi, C, N, k, stride, dil, pad, then ldx / ldy, Cm, splitk (0 = auto), the operand kind and how
the workspace is passed, and `expect`: (kernel, splitk, slab_tiles, nitems, fold launches) as csrc/conv_choice.h chooses for exactly
that descriptor -- tests/test_wgrad_refs.py feeds every descriptor to the header and asserts it, so a case that stops reaching its
kernel fails there, without a GPU.
"""
import numpy as np

from bn_cases import EPS32, F32, F64, bf16_round, h2_planes  # noqa: F401  (re-exported)

BK = 32                                         # pixel rows of one K step of every weight-gradient kernel
FOLD_CAP = 524288                               # threads of the largest fold grid
EINVAL = -1

R_X3 = 2 * 2.0 ** -24 + 2.0 ** -32
R_H2 = 3 * 2.0 ** -22 + 2.0 ** -44

PLAIN_BF16, PLAIN_F32 = "conv_wgrad_kernel<bf16>", "conv_wgrad_kernel<f32>"
X3, X3_LIN = "conv_wgrad_x3_kernel<0>", "conv_wgrad_x3_kernel<1>"
H2, H2_LIN = "conv_wgrad_h2_kernel<0>", "conv_wgrad_h2_kernel<1>"
WS, WS_LIN = "conv_wgrad_ws_kernel<0>", "conv_wgrad_ws_kernel<1>"
N64, BIG = "conv_wgrad_n64_kernel", "conv_wgrad_big_kernel<2>"
ALL_KERNELS = {PLAIN_BF16, PLAIN_F32, X3, X3_LIN, H2, H2_LIN, WS, WS_LIN, N64, BIG}


class Case:
    """kind: "bf16" | "f32" (f32_split 0) | "x3" (f32_split 1) | "planes" (f32_split 2 with both plane pairs);
    ws: "ws" (aligned workspace of ws_planes slabs) | "atomics" (none) | "misaligned" (the pointer 4 bytes past a 16-byte boundary);
    ws_elems overrides the capacity in floats; rc: the return code expected (0, or EINVAL: nothing may be written); mid: the exact inputs
    carry a second split term (see the module docstring)"""

    def __init__(self, cid, shape, ld, expect, Cm=0, splitk=0, kind="bf16", ws="ws", ws_planes=None, ws_elems=None, scaled=False, rc=0,
                 mid=False):
        self.id, self.mid = cid, mid
        self.B, self.Hi, self.Wi, self.C, self.N, self.k, self.stride, self.dil, self.pad = shape
        self.ldx, self.ldy = ld
        self.Cm, self.splitk, self.kind, self.ws, self.scaled, self.rc = Cm, splitk, kind, ws, scaled, rc
        self.Ho = (self.Hi + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        self.Wo = (self.Wi + 2 * self.pad - self.dil * (self.k - 1) - 1) // self.stride + 1
        self.M = self.B * self.Ho * self.Wo
        self.tiles = -(-self.M // BK)
        self.Ktot = self.k * self.k * self.C
        self.plane = self.N * self.Ktot                       # floats of one workspace slab
        self.cm = Cm if Cm > 0 else self.C
        self.dtype = "bf16" if kind == "bf16" else "f32"
        if ws == "atomics":
            self.ws_elems = 0
        elif ws_elems is not None:
            self.ws_elems = ws_elems
        else:
            self.ws_elems = (ws_planes if ws_planes is not None else (splitk if splitk > 0 else min(self.tiles, 256))) * self.plane
        self.kernel, self.x_splitk, self.x_slab, self.x_nitems, self.x_nreduce = expect
        assert self.M <= 18432 and self.C <= self.ldx and self.N <= self.ldy

    def __repr__(self):
        return self.id

    def shape(self):
        return (self.B, self.Hi, self.Wi, self.C, self.N, self.k, self.stride, self.dil, self.pad)

    def offsets(self, place):
        """channel offsets of the x and dy slices in their buffers"""
        return (0, 0) if place == "first" else (self.ldx - self.C, self.ldy - self.N)

    def desc(self):
        """the descriptor as tests/test_conv_choice.py's table writes one (a pointer: 0 = null, 16 + its low four address bits)"""
        d = dict(x=16, dy=16, dw=16, B=self.B, Hi=self.Hi, Wi=self.Wi, C=self.C, ldx=self.ldx, Ho=self.Ho, Wo=self.Wo, N=self.N,
                 ldy=self.ldy, R=self.k, S=self.k, stride=self.stride, dil=self.dil, pad=self.pad, dtype=1 if self.kind == "bf16" else 0,
                 splitk=self.splitk, Cm=self.Cm, ws={"ws": 16, "atomics": 0, "misaligned": 20}[self.ws], ws_elems=self.ws_elems,
                 f32_split={"bf16": 0, "f32": 0, "x3": 1, "planes": 2}[self.kind])
        if self.kind == "planes":
            d.update(x_planes=16, dy_planes=16, x_unscale=16, dy_unscale=16, x_plane_stride=self.B * self.Hi * self.Wi * self.ldx,
                     dy_plane_stride=self.M * self.ldy)
        return d


STRADDLE = (3, 7, 5, 40, 136, 3, 1, 1, 1)
WS128 = (2, 17, 16, 40, 128, 3, 1, 1, 1)
C120 = (2, 17, 16, 120, 256, 3, 1, 1, 1)
STEM = (2, 33, 27, 8, 64, 7, 2, 1, 3)

CASES = [
    # --- PLAIN, X3, N64 -------------------------------------------------------------------------------------------------------
    # 2 x 3 tiles; C = 40 does not divide 128: a tile's columns straddle tap boundaries; N and Ktot = 360 ragged; M = 105
    Case("plain_bf16_straddle", STRADDLE, (48, 144), (PLAIN_BF16, 1, 4, 0, 1), scaled=True),
    Case("plain_bf16_atomics_auto", STRADDLE, (48, 144), (PLAIN_BF16, 1, 4, 0, 0), ws="atomics"),
    Case("plain_bf16_atomics_sk3", STRADDLE, (48, 144), (PLAIN_BF16, 2, 2, 0, 0), ws="atomics", splitk=3),
    Case("plain_f32", (3, 7, 5, 20, 132, 3, 1, 1, 1), (24, 136), (PLAIN_F32, 1, 4, 0, 1), Cm=17, kind="f32", scaled=True),
    Case("x3_f32", (3, 7, 5, 20, 132, 3, 1, 1, 1), (24, 136), (X3, 1, 4, 0, 1), Cm=17, kind="x3", scaled=True),
    # exact inputs with a non-zero mid term: the cross products of the three-term split must all be there (M = 25)
    Case("x3_mid_terms", (1, 5, 5, 20, 132, 3, 1, 1, 1), (24, 136), (X3, 1, 1, 0, 1), Cm=17, kind="x3", mid=True),
    Case("plain_1x1_s2", (2, 9, 7, 40, 136, 1, 2, 1, 0), (48, 144), (PLAIN_BF16, 1, 2, 0, 1)),      # 1 x 1 stride 2 is not `lin`
    # one pixel; one short of, exactly, and one past a 32-pixel tile
    Case("m1", (1, 1, 1, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 1, 1, 0, 1)),
    Case("m31", (1, 1, 31, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 1, 1, 0, 1)),
    Case("m32", (1, 1, 32, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 1, 1, 0, 1)),
    Case("m33", (1, 1, 33, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 1, 2, 0, 1)),
    Case("m33_3x3", (1, 1, 33, 8, 8, 3, 1, 1, 1), (16, 16), (N64, 1, 2, 0, 1)),      # a one-row image: 6 of 9 taps are padding everywhere
    Case("n64_n24", (3, 7, 5, 40, 24, 3, 1, 1, 1), (48, 32), (N64, 1, 4, 0, 1), scaled=True),      # 2 k-blocks of 256, the second 104 wide
    Case("n64_s2_cm", (2, 9, 7, 40, 64, 3, 2, 1, 1), (48, 72), (N64, 1, 2, 0, 1), Cm=35),
    Case("n64_1x1_is_plain", (2, 5, 7, 40, 64, 1, 1, 1, 0), (48, 72), (PLAIN_BF16, 1, 3, 0, 1)),
    Case("stem_odd_bf16", STEM, (16, 72), (N64, 2, 8, 0, 1), Cm=3),                    # 49 taps of 8 channels, 15 tiles
    Case("stem_odd_planes", STEM, (16, 72), (H2, 2, 8, 0, 1), kind="planes"),
    Case("d6_on_5x5", (2, 5, 5, 32, 64, 3, 1, 6, 6), (40, 72), (N64, 1, 2, 0, 1)),     # 8 of 9 taps only ever see padding
    # --- H2, WS ---------------------------------------------------------------------------------------------------------------
    Case("h2_n136", STRADDLE, (48, 144), (H2, 1, 4, 0, 1), kind="planes", scaled=True),
    Case("h2_fewtiles", (2, 5, 7, 64, 128, 1, 1, 1, 0), (72, 136), (H2_LIN, 1, 3, 0, 1), kind="planes"),     # N % 128 == 0 but 3 tiles
    Case("h2_atomics", WS128, (48, 136), (H2, 3, 6, 0, 0), kind="planes", ws="atomics"),
    Case("h2_misaligned_ws", WS128, (48, 136), (H2, 3, 6, 0, 1), kind="planes", ws="misaligned"),       # falls from WS to H2
    Case("ws_n128_auto", WS128, (48, 136), (WS, 1, 17, 2, 1), kind="planes", scaled=True),          # 1 split, 2 items
    Case("ws_n128_sk5", WS128, (48, 136), (WS, 5, 4, 10, 1), kind="planes", splitk=5),              # slabs of 4, the last of 1 tile
    Case("ws_d2", (2, 17, 16, 40, 128, 3, 1, 2, 2), (48, 136), (WS, 3, 6, 6, 1), kind="planes", splitk=3),
    Case("ws_lin", (2, 17, 16, 264, 128, 1, 1, 1, 0), (272, 136), (WS_LIN, 1, 17, 2, 1), kind="planes"),   # second k-block 8 columns wide
    # 264 / 264 / 280 items on 256 persistent workgroups: one, two and four K steps per item (the ring has three stages)
    Case("ws_items_kt1", (2, 28, 25, 64, 256, 3, 1, 1, 1), (72, 264), (WS, 44, 1, 264, 1), kind="planes", splitk=44),
    Case("ws_items_kt2", (2, 28, 25, 64, 512, 3, 1, 1, 1), (72, 520), (WS, 22, 2, 264, 1), kind="planes", splitk=22),
    # slabs of 4 with the last of 3; 589824 fold elements: the fold grid strides at 64 threads per block
    Case("ws_items_kt4", (2, 22, 40, 128, 512, 3, 1, 1, 1), (136, 520), (WS, 14, 4, 280, 1), kind="planes", splitk=14),
    # --- BIG ------------------------------------------------------------------------------------------------------------------
    # 5 k-blocks, the last 56 wide; slabs of 9, of 3 (the last 2) and of 1 tile
    Case("big_c120_auto", C120, (128, 264), (BIG, 2, 9, 0, 1), Cm=117, ws_planes=4, scaled=True),
    Case("big_c120_sk6", C120, (128, 264), (BIG, 6, 3, 0, 1), Cm=117, splitk=6),
    Case("big_c120_sk17", C120, (128, 264), (BIG, 17, 1, 0, 1), Cm=117, splitk=17),
    Case("big_1x1", (2, 17, 16, 520, 512, 1, 1, 1, 0), (528, 520), (BIG, 2, 9, 0, 1), ws_planes=4),       # `lin`, 2 x 3 tiles
    Case("big_s2_odd", (2, 33, 35, 104, 256, 3, 2, 1, 1), (112, 264), (BIG, 2, 10, 0, 1), ws_planes=4),   # stride 2, odd image, 20 tiles
    Case("big_fold_stride", (2, 17, 16, 232, 256, 3, 1, 1, 1), (240, 264), (BIG, 2, 9, 0, 1), ws_planes=4),   # 534528 fold elements
    # --- chunked fold, workspace capacity ------------------------------------------------------------------------------------------
    Case("fold_64", (1, 32, 64, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 64, 1, 0, 1), splitk=64),
    Case("fold_65", (1, 45, 46, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 65, 1, 0, 2), splitk=65),      # a last chunk of 1
    Case("fold_67", (1, 45, 47, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 67, 1, 0, 2), splitk=67),      # chunks of 16, 16, 16, 16, 3
    Case("fold_67_cm5", (1, 45, 47, 8, 8, 1, 1, 1, 0), (16, 16), (PLAIN_BF16, 67, 1, 0, 2), splitk=67, Cm=5),
    Case("fold_x3_67", (1, 45, 47, 8, 12, 1, 1, 1, 0), (16, 16), (X3_LIN, 67, 1, 0, 2), splitk=67, kind="x3"),
    Case("fold_h2_67", (1, 45, 47, 8, 8, 1, 1, 1, 0), (16, 16), (H2_LIN, 67, 1, 0, 2), splitk=67, kind="planes"),
    Case("fold_80_n64", (2, 40, 32, 8, 8, 3, 1, 1, 1), (16, 16), (N64, 80, 1, 0, 2), splitk=80),         # five full chunks
    Case("fold_auto", (2, 96, 96, 64, 64, 1, 1, 1, 0), (72, 72), (PLAIN_BF16, 72, 8, 0, 2)),             # layer1's own shape class
    Case("ws_clamps", STRADDLE, (48, 144), (PLAIN_BF16, 2, 2, 0, 1), splitk=4, ws_planes=2),
    Case("ws_too_small", STRADDLE, (48, 144), (None, 0, 0, 0, 0), splitk=4, ws_elems=136 * 360 - 1, rc=EINVAL),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)

# The grouped launch: jobs are BIG shapes, pitched, with and without Cm; the workspace holds exactly the floats wgrad_group_choose
# partitions (GROUP_WS: asserted against the header by tests/test_wgrad_refs.py), and one float fewer is refused.
# a job: (single-launch case whose shape and pitches it takes, Cm); expect per job: (splitk, slab_tiles)
GROUPS = {
    "group_1": [("big_c120_auto", 117)],
    "group_12": [("big_c120_auto", 117), ("big_1x1", 0), ("big_s2_odd", 0), ("big_fold_stride", 0),
                 ("big_c120_auto", 0), ("big_1x1", 513), ("big_s2_odd", 97), ("big_fold_stride", 229),
                 ("big_c120_auto", 120), ("big_1x1", 8), ("big_s2_odd", 104), ("big_fold_stride", 1)],
}
GROUP_EXPECT = {
    "group_1": [(2, 9)],
    "group_12": [(2, 9), (2, 9), (2, 10), (2, 9)] * 3,
}
GROUP_WS = {"group_1": 552960, "group_12": 7901184}


def group_jobs(gid):
    """the jobs of a group as cases of their own (kind bf16, expect = the group's split of that job)"""
    out = []
    for j, ((cid, Cm), (sk, slab)) in enumerate(zip(GROUPS[gid], GROUP_EXPECT[gid])):
        b = BY_ID[cid]
        out.append(Case("%s.job%d" % (gid, j), b.shape(), (b.ldx, b.ldy), (BIG, sk, slab, 0, 1), Cm=Cm, ws_planes=sk))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
def _seed(case, kind):
    return (sum(ord(ch) * (i + 1) for i, ch in enumerate(case.id)) * 2 + (kind == "real")) % (2 ** 31)


def inputs(case, kind):
    """(x [B][Hi][Wi][C], dy [B][Ho][Wo][N], dw0 [N][k][k][Cm]) as float32 values the case's buffers hold exactly"""
    rs = np.random.RandomState(_seed(case, kind))
    xs, ys, ws = (case.B, case.Hi, case.Wi, case.C), (case.B, case.Ho, case.Wo, case.N), (case.N, case.k, case.k, case.cm)
    if kind == "exact" and case.mid:
        def two_terms(shape):
            return (rs.choice([-3, -2, 2, 3], shape) + rs.choice([-1, 1], shape) * 2.0 ** -8).astype(F32)
        return two_terms(xs), two_terms(ys), rs.randint(-8, 9, ws).astype(F32)
    if kind == "exact":
        return (rs.randint(-3, 4, xs).astype(F32), rs.randint(-3, 4, ys).astype(F32), rs.randint(-8, 9, ws).astype(F32))
    x, dy, dw0 = rs.standard_normal(xs).astype(F32), rs.standard_normal(ys).astype(F32), rs.standard_normal(ws).astype(F32)
    if case.scaled:
        x, dy, dw0 = x * F32(1e3), dy * F32(1e-4), dw0 * F32(0.1)
    if case.dtype == "bf16":
        x, dy = bf16_round(x), bf16_round(dy)
    return x, dy, dw0


# ---------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------
def wgrad_sum(x, dy, k, stride, dil, pad, dtype=F64):
    """sum over (b, yo, xo) of dy[b, yo, xo, n] * x[b, yo stride - pad + r dil, xo stride - pad + s dil, c] -> [N][k][k][C]"""
    x, dy = np.asarray(x, dtype), np.asarray(dy, dtype)
    Ho, Wo = dy.shape[1:3]
    xp = np.pad(x, ((0, 0), (pad, pad), (pad, pad), (0, 0)))
    out = np.zeros((dy.shape[3], k, k, x.shape[3]), dtype)
    for r in range(k):
        for s in range(k):
            win = xp[:, r * dil:r * dil + (Ho - 1) * stride + 1:stride, s * dil:s * dil + (Wo - 1) * stride + 1:stride, :]
            assert win.shape[:3] == dy.shape[:3]
            out[:, r, s, :] = np.tensordot(dy, win, axes=([0, 1, 2], [0, 1, 2]))
    return out


def wgrad_ref(case, x, dy, dw0):
    return np.asarray(dw0, F64) + wgrad_sum(x, dy, case.k, case.stride, case.dil, case.pad)[..., :case.cm]


def wgrad_mag(case, x, dy, dw0):
    """|dw0| + sum |dy * x|"""
    return np.abs(np.asarray(dw0, F64)) + wgrad_sum(np.abs(np.asarray(x, F64)), np.abs(np.asarray(dy, F64)), case.k, case.stride, case.dil,
                                                    case.pad)[..., :case.cm]


def wgrad_chain(case):
    """terms on the longest chain of additions: the pixel rows of a slab, the slabs, the value dw held"""
    return BK * case.x_slab + case.x_splitk + 1


def wgrad_r(case):
    if case.kernel in (X3, X3_LIN):
        return R_X3
    if case.kernel in (H2, H2_LIN, WS, WS_LIN):
        return R_H2
    return 0.0


def wgrad_bar(case, x, dy, dw0):
    return (wgrad_chain(case) * EPS32 + wgrad_r(case)) * wgrad_mag(case, x, dy, dw0)


def wgrad_f32(case, x, dy, dw0):
    """the reference evaluated in float32 in the kernels' structure: every slab of 32 * slab_tiles pixel rows summed on its own,
    the slabs added one after another, then the value dw held"""
    rows = BK * case.x_slab
    xf, yf = np.asarray(x, F32), np.asarray(dy, F32)
    # pixel index of every output position, to cut the sum into slabs
    m = np.arange(case.M).reshape(case.B, case.Ho, case.Wo)
    acc = np.zeros((case.N, case.k, case.k, case.C), F32)
    for s in range(case.x_splitk):
        keep = ((m >= s * rows) & (m < (s + 1) * rows))[..., None]
        acc = acc + wgrad_sum(xf, np.where(keep, yf, F32(0)), case.k, case.stride, case.dil, case.pad, F32)
    return (np.asarray(dw0, F32) + acc[..., :case.cm]).astype(F32)


# ---------------------------------------------------------------------------------------------------------------------
# the split formats, emulated
# ---------------------------------------------------------------------------------------------------------------------
def x3_terms(x):
    """the three-term bfloat16 split of conv_wgrad_x3_kernel: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)"""
    x = np.asarray(x, F32)
    hi = bf16_round(x)
    r = (x - hi).astype(F32)
    mid = bf16_round(r)
    lo = bf16_round((r - mid).astype(F32))
    return hi, mid, lo


def h2_scale(x):
    """dml_h2_split's s: the power of two that puts max |x| into [2^14, 2^15) (1 for a zero tensor)"""
    a = float(np.abs(x).max())
    return 1.0 if a == 0 else 2.0 ** (14 - int(np.floor(np.log2(a))))


def h2_terms(x):
    """(hi, lo, s): the two fp16 planes of s x"""
    s = h2_scale(x)
    hi, lo = h2_planes(x, 1.0 / s)
    return hi, lo, s
