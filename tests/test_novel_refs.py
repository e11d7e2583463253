"""CPU: the float64 definitions of tests/novel_cases.py are the reference's rules, the label tables of
Cityscapes.eval_relabel_lut are the reference's sequential passes, the seeded inputs keep the properties the GPU test
relies on, and the new entry points are declared and bound.  No kernel is launched here.

The reference lines restated below (test_embedding.py of the reference): :445 one novel class, :510-511 two, :520-522
three; the label shifts at :448-451, :512-517 and :523-530.
"""
import os

import numpy as np
import pytest

import helpers as H
import novel_cases as NC
import open_set_cases as CS


def _dis(feats_hwc, proto):
    """:430 -- -np.sum((features - prototype) ** 2, axis=1), reshaped to the image"""
    h, w, c = feats_hwc.shape
    return (-np.sum((feats_hwc.reshape(h * w, c) - proto) ** 2, axis=1)).reshape(h, w)


def _literal(N, preds, lg_khw, feats_hwc, protos, vs_known):
    """the reference's statements for one image, in float64, thresholds and labels as written there"""
    out = preds.copy()
    d = [_dis(feats_hwc.astype(np.float64), protos[j].astype(np.float64)) for j in range(N)]
    if N == 1:
        assert vs_known                                                  # :445
        out[np.logical_and(d[0] > -1.5, d[0] > lg_khw.astype(np.float64).max(axis=0))] = 16
        return out
    assert not vs_known
    if N == 2:                                                           # :510-511
        out[np.logical_and(d[0] > -1.5, d[0] > d[1])] = 16
        out[np.logical_and(d[1] > -1.5, d[1] > d[0])] = 17
        return out
    out[np.logical_and(d[0] > -1.5, np.logical_and(d[0] > d[1], d[0] > d[2]))] = 16    # :520-522
    out[np.logical_and(d[1] > -1.5, np.logical_and(d[1] > d[0], d[1] > d[2]))] = 17
    out[np.logical_and(d[2] > -1.5, np.logical_and(d[2] > d[1], d[2] > d[0]))] = 18
    return out


@pytest.mark.parametrize("N", (1, 2, 3))
def test_definition_is_the_reference_rule(N):
    feats, lg, protos, labels = NC.random_batch(N)
    vs_known = N == 1
    ref = NC.post_ref(lg, feats, protos, labels, -1.5, vs_known)
    rp, _ = CS.msp_ref(lg)
    for b in range(lg.shape[0]):
        assert np.array_equal(ref["preds"][b], _literal(N, rp[b], lg[b], feats[b], protos, vs_known))
        if N == 1:
            via, _, _ = CS.relabel_ref(rp[b], lg[b], feats[b], protos[0], -1.5, 16)
            assert np.array_equal(ref["preds"][b], via)


def test_definition_on_the_exact_row():
    """the situations the row was built for, and the literal rules on it (N = 3 with vs_known = False)"""
    feats, lg, protos, labels, what = NC.exact_row(16, 16)
    for b, order in ((0, slice(None)), (1, slice(None, None, -1))):
        r = {k: NC.post_ref(lg, feats, protos, labels, -1.5, k)["preds"][b, 0][order] for k in (True, False)}
        base = np.argmax(lg[b], axis=0)[0][order]
        assert np.array_equal(r[False], _literal(3, base[None], lg[b][:, :, order], feats[b][:, order], protos, False)[0])
        for k in (True, False):
            assert r[k][what["tie"]] == base[what["tie"]] and r[k][what["far"]] == base[what["far"]]
            assert r[k][what["on_thresh"]] == base[what["on_thresh"]]
            assert r[k][what["above"]] == 16 and r[k][what["p1"]] == 17 and r[k][what["p2"]] == 18
        assert r[True][what["on_logit"]] == base[what["on_logit"]] and r[False][what["on_logit"]] == 16
        assert r[True][what["zero"]] == base[what["zero"]] and r[False][what["zero"]] == 17
    ref = NC.post_ref(lg, feats, protos, labels, -1.5, True)
    assert ref["tie"][0, 0, what["tie"]] and ref["tie"].sum() == 2
    below = NC.post_ref(lg, feats, protos, labels, CS.down(-1.5), True)["preds"]
    above = NC.post_ref(lg, feats, protos, labels, CS.up(-1.5), True)["preds"]
    assert below[0, 0, what["on_thresh"]] == 16 and above[0, 0, what["on_thresh"]] != 16
    assert np.array_equal(ref["preds"][1], ref["preds"][0][:, ::-1])


@pytest.mark.parametrize("N", NC.RANDOM_NS)
def test_random_batch_cannot_degenerate(N):
    """at most 3.3e-5 of the pixels inside the fp32 margin (far below EXCLUDE_CAP), 22 .. 23 % relabelled, every prototype
    wins at least 2.6 % of the pixels"""
    feats, lg, protos, labels = NC.random_batch(N)
    assert feats.shape == (2, 96, 160, 16) and lg.shape == (2, 16, 96, 160) and protos.shape == (N, 16)
    for vs_known in (True, False):
        ref = NC.post_ref(lg, feats, protos, labels, -1.5, vs_known)
        assert 1.0 - ref["sure"].mean() <= 3.3e-5 < CS.EXCLUDE_CAP
    ref = NC.post_ref(lg, feats, protos, labels, -1.5, True)
    assert 0.22 <= ref["hit"].mean() <= 0.23
    for j in range(N):
        assert (ref["hit"] & (ref["jstar"] == j)).mean() >= 0.026
        assert (ref["preds"] == labels[j]).sum() == (ref["hit"] & (ref["jstar"] == j)).sum()


def test_no_prototype_is_plain_argmax():
    feats, lg, protos, labels = NC.random_batch(0, 13, 19, (3, 5, 7))
    assert protos is None and labels == []
    ref = NC.post_ref(lg, feats, protos, labels, -1.5, True)
    assert np.array_equal(ref["preds"], CS.msp_ref(lg)[0]) and ref["sure"].all()


def _sequential(n_held):
    """:448-451, :512-517, :523-530 applied to all 256 ids with numpy, statement by statement"""
    labels = np.arange(256, dtype=np.int64)
    if n_held == 1:
        labels[labels == 13] = -1
        labels[labels >= 14] -= 1
        labels[labels == -1] = 16
        labels[labels == 254] = 255
    elif n_held == 2:
        labels[labels == 13] = -2
        labels[labels == 14] = -1
        labels[labels >= 15] -= 2
        labels[labels == -2] = 16
        labels[labels == -1] = 17
        labels[labels == 253] = 255
    else:
        labels[labels == 13] = -3
        labels[labels == 14] = -2
        labels[labels == 15] = -1
        labels[labels >= 16] -= 3
        labels[labels == -3] = 16
        labels[labels == -2] = 17
        labels[labels == -1] = 18
        labels[labels == 252] = 255
    return labels.astype(np.uint8)


def test_label_tables_are_the_sequential_passes():
    from datasets.cityscapes import Cityscapes
    assert np.array_equal(Cityscapes.eval_relabel_lut(), _sequential(1))
    assert np.array_equal(Cityscapes.eval_relabel_lut(13, 16), _sequential(1))
    assert np.array_equal(Cityscapes.eval_relabel_lut([13], [16]), _sequential(1))
    assert np.array_equal(Cityscapes.eval_relabel_lut((13, 14), (16, 17)), _sequential(2))
    assert np.array_equal(Cityscapes.eval_relabel_lut([13, 14, 15], [16, 17, 18]), _sequential(3))
    # the order of the pairs does not matter; 255 stays 255; the int form is what it was for another class
    assert np.array_equal(Cityscapes.eval_relabel_lut((15, 13, 14), (18, 16, 17)), _sequential(3))
    t = np.arange(256, dtype=np.int64)
    old = np.where(t > 5, t - 1, t)
    old[5] = 18
    old[old == 254] = 255
    assert np.array_equal(Cityscapes.eval_relabel_lut(5, 18), old.astype(np.uint8))
    with pytest.raises(ValueError):
        Cityscapes.eval_relabel_lut((13, 14), (16,))
    with pytest.raises(ValueError):
        Cityscapes.eval_relabel_lut((13, 13), (16, 17))


def test_entry_points_are_declared_and_bound():
    from dmlnet import _lib
    header = open(os.path.join(H.ROOT, "include", "dmlnet_hip.h")).read()
    for name in ("dml_open_world_post", "dml_class_feature_sums"):
        assert name in _lib.EXPORTS and ("int %s(" % name) in header
    lib = _lib.load()
    assert lib.dml_abi_version() == 6
    for name in ("dml_open_world_post", "dml_novel_relabel_multi", "dml_class_feature_sums"):
        fid = lib.dml_plan_fn_id(name.encode())
        assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(getattr(lib, name).argtypes) - 1, name
    # argument checks return before any HIP call
    assert lib.dml_open_world_post(None, None, None, None, None, None, None, None, 1, 16, 16, 4, 4, 0, -1.5, 1, 1000.0, 0,
                                   None) == -1
    assert lib.dml_class_feature_sums(None, None, 4, 16, None, 1, None, None, None) == -1


def test_driver_parser_takes_several_prototype_files():
    import eval_open_world as T
    p = T.build_parser()
    o = p.parse_args(["--synthetic", "--prototype_json", "a.json", "b.json", "c.json", "--novel_only"])
    assert o.prototype_json == ["a.json", "b.json", "c.json"] and o.novel_only
    o = p.parse_args(["--synthetic", "--prototype_json", "a.json"])
    assert o.prototype_json == ["a.json"] and not o.novel_only and o.extract_prototypes is None
    o = p.parse_args(["--synthetic", "--extract_prototypes", "13", "14", "--shots_out", "shots"])
    assert o.extract_prototypes == [13, 14] and o.shots_out == "shots"
    assert p.parse_args(["--synthetic"]).prototype_json is None


def test_python_surface_is_exported():
    import inspect
    import utils
    sig = inspect.signature(utils.open_world_post)
    assert list(sig.parameters) == ["logits", "feats", "protos", "new_labels", "thresh", "vs_known", "clip", "inclusive",
                                    "want_msp", "want_score"]
    assert sig.parameters["thresh"].default == -1.5 and sig.parameters["vs_known"].default is True
    assert list(inspect.signature(utils.novel_relabel_multi).parameters) == ["preds", "logits", "feats", "protos",
                                                                             "new_labels", "thresh", "vs_known"]
    assert list(inspect.signature(utils.extract_prototypes).parameters) == ["features", "labels_true", "class_ids",
                                                                            "min_fraction"]
