"""CPU: the float64 definition of tests/knn_cases.py is the reference's `--ood knn` branch, the bar holds for a float32
evaluation of the reference's own statements, the seeded inputs keep the properties the GPU test relies on, and the new
entry point is declared and bound.  No kernel is launched here.

The reference lines restated below (anomaly/eval_ood_traditional.py of the reference): :512 neighbor_size = 9, :514 the
zero map, :518-519 the two shift loops from 1 to neighbor_size - 1, :520-522 the zero-filled copy shifted up-left and its
cosine similarity over the channel axis, :523-525 the copy shifted down-right.  The resize at :527 is the identity on a
map that already has segSize, and the plot at :526-529 is not part of the score.
"""
import os

import numpy as np
import pytest
import torch

import helpers as H
import knn_cases as KC

# shapes with H, W >= R, where the reference's slices are defined
LITERAL = [name for name, ((B, C, Hh, Ww), ns, _) in KC.CASES.items() if Hh >= ns - 1 and Ww >= ns - 1]


def _literal(ft1, neighbor_size, dtype):
    """:512-525 for one image ft1 [C, H, W], in `dtype`"""
    ft1 = torch.from_numpy(np.array(ft1)).to(dtype)              # a writable copy
    cosdis_map = torch.zeros(ft1.shape[1:], dtype=dtype)                                            # :514
    c, h, w = ft1.shape
    for shift_h in range(1, neighbor_size):                                                         # :518
        for shift_w in range(1, neighbor_size):                                                     # :519
            shifted = torch.zeros_like(ft1)
            shifted[:, 0:(h - shift_h), 0:(w - shift_w)] = ft1[:, shift_h:h, shift_w:w]             # :521
            cosdis_map += torch.nn.functional.cosine_similarity(ft1, shifted, dim=0)                # :522
            shifted = torch.zeros_like(ft1)
            shifted[:, shift_h:h, shift_w:w] = ft1[:, 0:(h - shift_h), 0:(w - shift_w)]             # :524
            cosdis_map += torch.nn.functional.cosine_similarity(ft1, shifted, dim=0)                # :525
    return cosdis_map.numpy()


def test_literal_list_covers_the_table():
    assert {"size_R", "size_R1", "c1", "c32_big", "seams", "scalar", "ns1", "ns2", "ns17", "vec_seams"} <= set(LITERAL)
    assert not {"one_pixel", "short", "narrow"} & set(LITERAL)


@pytest.mark.parametrize("name", LITERAL)
def test_definition_is_the_reference_branch(name):
    feats, score, T = KC.reference(name)
    ns = KC.CASES[name][1]
    for b in range(feats.shape[0]):
        lit = _literal(feats[b], ns, torch.float64)
        err = np.abs(lit - score[b]).max()
        print("MEASURE literal f64 %s img %d err=%.3e bar=%.3e" % (name, b, err, 1e-12))
        assert err <= 1e-12


@pytest.mark.parametrize("name", LITERAL)
def test_float32_statements_stay_within_the_bar(name):
    feats, score, T = KC.reference(name)
    ns = KC.CASES[name][1]
    for b in range(feats.shape[0]):
        lit = _literal(feats[b], ns, torch.float32).astype(np.float64)
        excess = np.abs(lit - score[b]) - KC.bar(T[b])
        ratio = (np.abs(lit - score[b]) / np.maximum(KC.bar(T[b]), 1e-300)).max()
        print("MEASURE literal f32 %s img %d err=%.3e bar=%.3e worst err/bar=%.3e"
              % (name, b, np.abs(lit - score[b]).max(), KC.bar(T[b]).max(), ratio))
        assert (excess <= 0).all()


def test_small_images_and_size_one():
    """what the reference cannot run: an image smaller than the neighbourhood only loses the neighbours outside it, one
    pixel and neighbor_size = 1 give zeros"""
    f, s, T = KC.reference("one_pixel")
    assert s.shape == (1, 1, 1) and s[0, 0, 0] == 0.0 and T[0, 0, 0] == 0.0
    f, s, T = KC.reference("ns1")
    assert not s.any() and not T.any()
    # brute force over the pixels of the short and the narrow image
    for name in ("short", "narrow"):
        f, s, T = KC.reference(name)
        f64 = f.astype(np.float64)[0]
        n = f64 / np.maximum(np.sqrt((f64 * f64).sum(axis=0)), KC.CLAMP)
        _, Hh, Ww = n.shape
        want = np.zeros((Hh, Ww))
        for y in range(Hh):
            for x in range(Ww):
                for i in range(1, 9):
                    for j in range(1, 9):
                        for yy, xx in ((y + i, x + j), (y - i, x - j)):
                            if 0 <= yy < Hh and 0 <= xx < Ww:
                                want[y, x] += n[:, y, x] @ n[:, yy, xx]
        assert np.abs(want - s[0]).max() <= 1e-12


def test_c1_yields_integers():
    f, s, T = KC.reference("c1")
    assert np.array_equal(s, np.round(s)) and np.abs(s).max() >= 8
    for b in range(f.shape[0]):
        assert np.array_equal(_literal(f[b], 9, torch.float32).astype(np.float64), s[b])


@pytest.mark.parametrize("name", sorted(KC.CASES))
def test_inputs_keep_their_properties(name):
    (B, C, Hh, Ww), ns, flavour = KC.CASES[name]
    f, s, T = KC.reference(name)
    assert f.shape == (B, C, Hh, Ww) and f.dtype == np.float32 and np.isfinite(f).all() and np.abs(f).max() <= 1e18
    assert C <= KC.MAXC and 1 <= ns <= KC.MAX_NEIGHBOR_SIZE
    norms = np.sqrt((f.astype(np.float64) ** 2).sum(axis=1))
    if Hh >= 2 and Ww >= 2:
        zero = norms == 0.0
        assert zero.any() and not s[zero].any()                  # zero vectors are present and score exactly 0
    if ns >= 2 and Hh >= 2 and Ww >= 2:
        assert (T > 0).any()
    if flavour == "subeps":
        sub = (norms > 0.0) & (norms < KC.CLAMP)
        assert sub.sum() >= 100 and np.abs(s[sub]).max() > 0.0
    if flavour == "big":
        sq = (f.astype(np.float64) ** 2).sum(axis=1).max()
        assert 1e30 < sq < float(np.finfo(np.float32).max)       # large, and finite in fp32
    assert np.isfinite(s).all() and (np.abs(s) <= T + 1e-12).all()


def test_entry_point_is_declared_and_bound():
    from dmlnet import _lib
    header = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    assert "dml_knn_cosine_score" in _lib.EXPORTS and "int dml_knn_cosine_score(" in header
    lib = _lib.load()
    assert lib.dml_abi_version() == 6
    fid = lib.dml_plan_fn_id(b"dml_knn_cosine_score")
    assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(lib.dml_knn_cosine_score.argtypes) - 1
    # argument checks return before any HIP call
    assert lib.dml_knn_cosine_score(None, None, 1, 13, 4, 4, 9, None) == -1


def test_python_surface():
    import inspect
    import utils
    sig = inspect.signature(utils.knn_cosine_score)
    assert list(sig.parameters) == ["feats", "neighbor_size"] and sig.parameters["neighbor_size"].default == 9
    with pytest.raises(RuntimeError):
        utils.knn_cosine_score(torch.zeros(1, 13, 4, 4))             # no CPU fallback
    import eval_ood_traditional as T
    sig = inspect.signature(T.confidence)
    assert list(sig.parameters) == ["scores", "ood", "exclude_back", "feats"] and sig.parameters["feats"].default is None
    with pytest.raises(ValueError):
        T.confidence(torch.zeros(1, 14, 4, 4), "knn")
