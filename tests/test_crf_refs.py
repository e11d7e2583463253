"""CPU: the float64 definition of the Gaussian dense-CRF confidence (tests/crf_cases.py) is what it claims to be, the bars
of tests/test_gpu_crf_gauss.py have room for a correct float32 implementation, and the entry points, the wrapper and the
driver flags exist.  No kernel is launched here.

pydensecrf is not imported, here or anywhere in this suite: it is not a dependency of the project, and its permutohedral
lattice approximates the Gaussian filter that the definition states exactly, so the two do not agree digit for digit.
"""
import inspect
import os

import numpy as np
import pytest
import torch

import crf_cases as CC
import helpers as H

F64 = np.float64


def brute_force(L, sx, sy, compat, iters, clip=CC.CLIP):
    """the mean field with the full H W x H W kernel matrix and densecrf's symmetric normalisation, nothing factorised"""
    C, Hh, Ww = L.shape
    R_x, R_y = CC.radius(sx), CC.radius(sy)
    ys, xs = np.divmod(np.arange(Hh * Ww), Ww)
    dy, dx = ys[:, None] - ys[None, :], xs[:, None] - xs[None, :]
    K = np.exp(-dy.astype(F64) ** 2 / (2 * sy ** 2)) * np.exp(-dx.astype(F64) ** 2 / (2 * sx ** 2))
    K = np.where((np.abs(dy) <= R_y) & (np.abs(dx) <= R_x), K, 0.0)
    n = 1.0 / np.sqrt(K.sum(axis=1) + 1e-20)
    A = n[:, None] * K * n[None, :]
    U = CC.unary(L.astype(F64), clip).reshape(C, -1)
    Q = CC.softmax0(-U)
    for _ in range(iters):
        Q = CC.softmax0(-U + compat * (Q @ A.T))
    return Q.reshape(C, Hh, Ww)


@pytest.mark.parametrize("shape,sxy", [((3, 5, 7), (3.0, 3.0)), ((4, 9, 6), (3.0, 3.0)), ((4, 9, 6), (1.5, 0.7))])
def test_separable_definition_is_the_brute_force_mean_field(shape, sxy):
    L = CC.logits((1,) + shape, 2.0, 5)[0]
    for iters in (0, 1, 7):
        want = brute_force(L, sxy[0], sxy[1], 3.0, iters)
        got = CC.mean_field(L, sx=sxy[0], sy=sxy[1], compat=3.0, iters=iters)
        assert np.abs(got - want).max() <= 1e-12
        assert np.abs(got.sum(axis=0) - 1.0).max() <= 1e-12


def test_compat_zero_returns_q0():
    L = CC.logits((1, 13, 23, 37), 2.0, 6)[0]
    q0 = CC.mean_field(L, iters=0)
    p = np.clip(CC.softmax0(L.astype(F64)), CC.CLIP, 1.0)
    assert np.abs(q0 - p / p.sum(axis=0)).max() <= 1e-15             # the re-normalised clipped softmax
    for iters in (1, 5, 100):
        assert np.array_equal(CC.mean_field(L, compat=0.0, iters=iters), q0)


def test_constant_logits_give_a_constant_interior():
    R = CC.radius(3.0)
    Hh, Ww = 4 * R + 5, 4 * R + 7               # a pixel 2 R from the border sees only neighbours with a full kernel sum
    L = np.broadcast_to(np.linspace(-1.0, 2.0, 5, dtype=np.float32)[:, None, None], (5, Hh, Ww))
    Q = CC.mean_field(L, iters=1)
    inner = Q[:, 2 * R:Hh - 2 * R, 2 * R:Ww - 2 * R]
    assert np.abs(inner - inner[:, :1, :1]).max() <= 1e-14
    assert np.abs(Q[:, 0, 0] - inner[:, 0, 0]).max() > 1e-6          # and the border is not: fewer neighbours there
    # away from the border the kernel sums to the same value everywhere, so the message is Q itself
    Ax, Ay = CC.filters(Hh, Ww, 3.0, 3.0)
    q0 = CC.mean_field(L, iters=0)
    inner = (slice(None), slice(2 * R, Hh - 2 * R), slice(2 * R, Ww - 2 * R))
    assert np.abs(CC.message(q0, Ax, Ay)[inner] - q0[inner]).max() <= 1e-14


def test_one_hot_message_is_the_normalised_kernel():
    R = CC.radius(3.0)
    Hh = Ww = 4 * R + 1
    Q = np.zeros((1, Hh, Ww))
    Q[0, 2 * R, 2 * R] = 1.0
    Ax, Ay = CC.filters(Hh, Ww, 3.0, 3.0)
    M = CC.message(Q, Ax, Ay)[0]
    d = np.arange(-R, R + 1)
    k1 = np.exp(-d.astype(F64) ** 2 / 18.0)
    want = np.zeros((Hh, Ww))
    want[R:3 * R + 1, R:3 * R + 1] = np.outer(k1, k1) / k1.sum() ** 2
    assert np.abs(M - want).max() <= 1e-15
    assert M[2 * R, 2 * R] > 0                                        # the pixel's own term is included


def test_degenerate_axes_are_the_1d_filter():
    L = CC.logits((1, 6, 1, 40), 2.0, 7)[0]
    Q = CC.mean_field(L, iters=3)
    # H = 1: ky is the single tap 1 and ny = 1 -- the 1-D mean field along x
    K = CC.kernel_matrix(40, 3.0)
    n = 1.0 / np.sqrt(K.sum(axis=1))
    A = n[:, None] * K * n[None, :]
    U = CC.unary(L.astype(F64))
    q = CC.softmax0(-U)
    for _ in range(3):
        q = CC.softmax0(-U + 3.0 * (q[:, 0] @ A.T)[:, None, :])
    assert np.abs(Q - q).max() <= 1e-14
    # and the transposed frame gives the transposed result
    Qt = CC.mean_field(np.ascontiguousarray(L.transpose(0, 2, 1)), iters=3)
    assert np.abs(Qt.transpose(0, 2, 1) - Q).max() <= 1e-14


def test_truncation_at_six_sigma_is_below_1e_7():
    for name in ("odd_it100", "aniso_it5", "tiles_under_it5"):
        c = CC.CASES[name]
        lg, ref = CC.reference(name)
        full = CC.score_ref(lg, c["k_first"], sx=c["sx"], sy=c["sy"], compat=c["compat"], iters=c["iters"], R=None)
        err = np.abs(full["conf"] - ref["conf"]).max()
        print("MEASURE %s truncation err=%.3e" % (name, err))
        assert err < 1e-7


@pytest.mark.parametrize("name", sorted(CC.CASES))
def test_gpu_bars_have_margin(name):
    """a float32 numpy run of the definition stays within 1/8 of the GPU bar, and at most 1 % of the pixels are near-ties"""
    c = CC.CASES[name]
    lg, ref = CC.reference(name)
    f32 = CC.score_ref(lg, c["k_first"], sx=c["sx"], sy=c["sy"], compat=c["compat"], iters=c["iters"], dtype=np.float32)
    assert f32["conf"].dtype == np.float32
    err = np.abs(f32["conf"].astype(F64) - ref["conf"]).max()
    ties = ref["tie"].mean()
    moved = (f32["map"] != ref["map"])[~ref["tie"]].sum()
    print("MEASURE %s float32 err=%.3e (bar/8 = %.3e) ties=%.4f labels off outside ties=%d"
          % (name, err, CC.GPU_BAR / 8, ties, moved))
    assert err <= CC.GPU_BAR / 8
    assert ties <= 0.01
    assert moved == 0
    assert np.isfinite(ref["conf"]).all() and ref["conf"].min() >= 1.0 / (c["shape"][1] - c["k_first"]) - 1e-12


def test_cases_cover_what_they_claim():
    # the CRF does something on these inputs: labels change between Q^0 and Q^100
    c = CC.CASES["odd_it100"]
    lg, ref = CC.reference("odd_it100")
    q0 = CC.score_ref(lg, 0, iters=0)
    changed = (q0["map"] != ref["map"]).mean()
    print("MEASURE odd_it100 labels changed by the CRF: %.3f" % changed)
    assert 0.02 <= changed <= 0.5
    shapes = {n: v["shape"] for n, v in CC.CASES.items()}
    assert shapes["tiles_over_it5"][2:] == (33, 257) and shapes["tiles_under_it5"][2:] == (31, 255)
    assert shapes["c32_tiles_it5"][1:] == (32, 17, 65) and CC.CASES["kfirst_it100"]["k_first"] == 1
    assert CC.radius(CC.CASES["wide_it5"]["sx"]) == 48 and CC.radius(3.0) == 18 and CC.radius(1.5) == 9
    assert c["clip"] == 1e-5


def test_entry_points_wrapper_and_driver_flags_exist():
    from dmlnet import _lib
    header = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    assert "dml_crf_gauss" in _lib.EXPORTS and "dml_crf_gauss_workspace_bytes" in _lib.EXPORTS
    assert "int dml_crf_gauss(" in header and "int64_t dml_crf_gauss_workspace_bytes(" in header
    lib = _lib.load()
    assert lib.dml_abi_version() == 6
    fid = lib.dml_plan_fn_id(b"dml_crf_gauss")
    assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(lib.dml_crf_gauss.argtypes) - 1 == 14
    # the query is the header's formula, and both entry points refuse before any HIP call
    assert lib.dml_crf_gauss_workspace_bytes(2, 13, 70, 130) == 4 * (3 * 2 * 13 * 70 * 130 + 70 + 130 + 256)
    assert lib.dml_crf_gauss_workspace_bytes(1, 33, 4, 4) == -3 and lib.dml_crf_gauss_workspace_bytes(0, 13, 4, 4) == -1
    assert lib.dml_crf_gauss(None, None, None, None, 1, 13, 4, 4, 0, 3.0, 3.0, 3.0, 100, 1e-5, None) == -1

    import eval_ood_traditional as T
    opts = T.build_parser().parse_args(["--ood", "crf-gauss", "--crf_sxy", "2.5", "--crf_compat", "4", "--crf_iters", "7"])
    assert opts.ood == "crf-gauss" and opts.crf_sxy == 2.5 and opts.crf_compat == 4.0 and opts.crf_iters == 7
    opts = T.build_parser().parse_args(["--ood", "crf-gauss"])
    assert (opts.crf_sxy, opts.crf_compat, opts.crf_iters) == (3.0, 3.0, 100) == (T.CRF["sxy"], T.CRF["compat"], T.CRF["iters"])
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["--ood", "crf"])                 # the bilateral variant is not offered
    assert "crf-gauss" in T.__doc__ and "15-dimensional" in T.__doc__

    import utils
    sig = inspect.signature(utils.dense_crf_gauss)
    assert list(sig.parameters) == ["scores", "sxy", "compat", "iters", "first_class", "clip", "return_map"]
    d = {k: v.default for k, v in sig.parameters.items() if k != "scores"}
    assert d == {"sxy": 3.0, "compat": 3.0, "iters": 100, "first_class": 0, "clip": 1e-5, "return_map": False}
    with pytest.raises(RuntimeError):
        utils.dense_crf_gauss(torch.zeros(1, 13, 4, 4))               # a CPU tensor: no fallback
