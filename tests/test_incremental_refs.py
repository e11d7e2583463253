"""CPU: the references tests/test_gpu_incremental_predict.py holds the prediction kernel to (tests/incremental_cases.py) agree
with each other -- the fp64 rule built from the oracle's pieces, a literal restatement of the reference's lines
(test_self_distillation.py:292-297) and the fixture minted from the reference model itself -- and every seeded case keeps
its undecided share under the cap.  Host-side pieces of the feature (model classes, driver flags, binding) are checked here
too, so that they fail without a GPU."""
import os
import sys

import numpy as np
import pytest
import torch

import helpers as H
import incremental_cases as IC


@pytest.mark.parametrize("c", IC.CASES, ids=IC.case_id)
def test_rule_and_literal_restatement_agree(c):
    seed, shape, hs = c
    heads, ref = IC.case(seed, shape, hs)              # asserts the 1 % cap
    Ks, Cs, ids = hs
    B, Hh, Ww = shape[4], shape[2], shape[3]
    assert ref["pred"].shape == (B, Hh, Ww) and ref["pred"].dtype == torch.int64
    # the merge written out per pixel
    want = ref["argmax"][0].clone()
    for i in range(1, len(Ks)):
        want = torch.where(ref["argmax"][i] == ids[i], torch.full_like(want, ids[i]), want)
    assert torch.equal(want, ref["pred"])
    if Ks[0] == 16:                                    # the reference's head widths: its own lines apply
        lit = IC.merge_literal([lg.clone() for lg in ref["logits"]], len(Ks) - 1)
        assert torch.equal(lit, ref["pred"])
    # a float32 evaluation of the same rule agrees on every decided pixel
    ams = []
    for hd in heads:
        x = hd["e"][..., :hd["C"]].permute(0, 3, 1, 2).contiguous()
        from oracle import dmlnet_ref as O
        lg, _, _ = O.distance_head(O.bilinear(x, (Hh, Ww)), IC.centers(hd["K"], hd["C"], torch.float32))
        ams.append(IC.first_max(lg))
    p32 = IC.merge(ams, list(ids))
    assert torch.equal(p32[ref["decided"]], ref["pred"][ref["decided"]])


def test_padding_columns_and_k_equal_c_plus_one():
    # NaN columns beyond C never reach the reference; a K = C + 1 head's last prototype is the zero row
    heads, ref = IC.case(IC.SEED, (3, 5, 12, 20, 2), ((16, 17), (16, 24), (0, 16)), ld_extra=4)
    assert torch.isnan(heads[0]["e"][..., 16:]).all() and not torch.isnan(ref["logits"][0]).any()
    heads, ref = IC.case(IC.SEED, (3, 5, 12, 20, 2), ((33,), (32,), (0,)))
    assert (ref["argmax"][0] == 32).any() and (ref["argmax"][0] < 32).any()
    # argmax of d == argmax of f with 1.5 standing for the missing channel: the identity the kernel uses
    x = heads[0]["e"].double().permute(0, 3, 1, 2)
    from oracle import dmlnet_ref as O
    f = torch.cat([O.bilinear(x, (12, 20)), torch.full((2, 1, 12, 20), 1.5, dtype=torch.float64)], 1)
    assert torch.equal(IC.first_max(f)[ref["decided"]], ref["argmax"][0][ref["decided"]])


def test_g17_fixture_matches_the_rule():
    g = H.load_golden("g17_incremental")
    heads = [dict(e=torch.from_numpy(g["e0"]), C=16, K=16, ld=16, novel_id=0),
             dict(e=torch.from_numpy(g["e1"]), C=17, K=17, ld=17, novel_id=16)]
    assert heads[0]["e"].shape == (2, 16, 16, 16) and heads[1]["e"].shape == (2, 16, 16, 17)
    ref = IC.reference(heads, 64, 64)
    pred, dec = torch.from_numpy(g["pred"]).long(), torch.from_numpy(g["decided"]).bool()
    assert pred.shape == (2, 64, 64)
    assert torch.equal(dec, ref["decided"]) and 1.0 - dec.double().mean().item() <= IC.MAX_UNDECIDED
    assert torch.equal(pred[dec], ref["pred"][dec])
    over = (pred == 16).double().mean().item()
    assert over >= 0.01 and 1.0 - over >= 0.5


def test_model_classes_take_cls_novel_and_refuse_training_mode():
    import network
    from network import modeling as M
    m = M._segm_resnet("deeplabv3plus_embedding_self_distillation", "resnet50", None, 16, False, cls_novel=3)
    keys = list(m.state_dict().keys())
    for n, k in (("classifier", 16), ("classifier_1", 17), ("classifier_2", 18), ("classifier_3", 19)):
        assert m.state_dict()[n + ".classifier.3.weight"].shape[0] == k
    assert not any(k.startswith("classifier_4") for k in keys)
    assert m.classifier_list == ["classifier", "classifier_1", "classifier_2", "classifier_3"]
    d = network.deeplabv3plus_embedding_self_distillation_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
    assert d.classifier_list == ["classifier", "classifier_1"] and d.cls_novel == 1        # the default stays 1
    d.train()
    with pytest.raises(RuntimeError, match="eval"):
        d.predict(torch.zeros(1, 3, 64, 64))
    d.eval()
    with pytest.raises(ValueError):
        d.predict(torch.zeros(1, 3, 64, 64), novel_cls=2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        d.predict(torch.zeros(1, 3, 64, 64))           # no CPU path


def test_binding_and_plan_entry():
    import ctypes as C
    from dmlnet import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.PredictHead) == 24
    fid = lib.dml_plan_fn_id(b"dml_incremental_predict")
    assert fid >= 0 and lib.dml_plan_fn_nargs(fid) == len(lib.dml_incremental_predict.argtypes) - 1
    # argument checks run on the host: no launch happens for a rejected call
    hd = (_lib.PredictHead * 5)(*[_lib.PredictHead(16, 16, 16, 16, 16) for _ in range(5)])
    assert lib.dml_incremental_predict(None, 1, 16, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.dml_incremental_predict(hd, 1, None, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.dml_incremental_predict(hd, 0, 16, None, 1, 1, 1, 1, 1, None) == -1
    assert lib.dml_incremental_predict(hd, 5, 16, None, 1, 1, 1, 1, 1, None) == -3


def test_driver_parser_has_the_reference_flags():
    sys.path.insert(0, H.PKG)
    import importlib
    drv = importlib.import_module("test_self_distillation")
    o = drv.build_parser().parse_args(["--synthetic", "--novel_cls", "1", "--test_only", "--save_val_results",
                                       "--ckpt", "x.pth", "--gpu_id", "0", "--batch_size", "2", "--crop_val",
                                       "--dataset", "cityscapes", "--data_root", "/nowhere"])
    assert o.novel_cls == 1 and o.test_only and o.save_val_results and o.batch_size == 2
    assert o.model == "deeplabv3plus_embedding_self_distillation_resnet101" and o.num_classes == 16
