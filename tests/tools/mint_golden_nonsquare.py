#!/usr/bin/env python3
"""Mint the conditioning records of the live-oracle checks on inputs off the square / output-stride grid (authoring container only;
imports the real reference):

    g13n_nonsquare   deeplabv3plus_embedding_resnet101, 2 x 3 x 128 x 192, synth weights of seed 11
    g13o_offgrid     the same network, 2 x 3 x 97 x 129, synth weights of seed 13: every map is odd (97 x 129 -> 49 x 65 -> 25 x 33 ->
                     13 x 17 -> 7 x 9), H * W is odd and the final upsample is not x4

each with the BatchNorm betas moved so that no ReLU input of the network lies within 64 * eps32 * sum|terms| (and 6 x the reference's
own fp32-vs-fp64 noise) of zero -- the procedure and the proof of tests/tools/mint_golden_large.py, on other input shapes.

tests/test_gpu_model.py::test_against_oracle_nonsquare_strict / test_against_oracle_offgrid_strict run the HIP model AND the oracle (fp32
and fp64, at test time) on these weights; a fixture carries only the moved betas (sparse) and the proof numbers.  The 64 x 96 input the
non-square test used before normalises layer3 / layer4 / ASPP over 48 samples and sat on ReLU knife edges: its bar on the worst gradient
(5e-2) had been set around one sign flip, and any change of a convolution's summation order moved which element flips.

    python tests/tools/mint_golden_nonsquare.py [name ...] [--out DIR]     (~10 min per record on 8 cores; default: every record into
                                                                            tests/golden)
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "tools")]
sys.dont_write_bytecode = True
import helpers as H  # noqa: E402
import mint_golden as MG  # noqa: E402
import mint_golden_large as ML  # noqa: E402
from oracle import dmlnet_ref as O  # noqa: E402

# name, seed, input shape; the image is H.synth_tensor(seed, "<prefix>.img", shape), prefix = the name up to its first "_"
RECORDS = [
    ("g13n_nonsquare", 11, (2, 3, 128, 192)),
    ("g13o_offgrid", 13, (2, 3, 97, 129)),
]


def mint(R, name, seed, shape):
    def prep(m):
        m.train()
        m.classifier.aspp.project[3].eval()
        O.set_bn_momentum(m.backbone, 0.01)

    print("%s: input %s, conditioned weights (seed %d)" % (name, shape, seed))
    ctor = lambda: R.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)  # noqa: E731
    shapes = H.shapes_of(ctor())
    img = H.synth_tensor(seed, name.split("_")[0] + ".img", shape)
    sd, (bidx, bval), proof = ML.condition(ctor, shapes, seed, img, prep)
    chk = H.conditioned_state_dict(shapes, seed, bidx.numpy(), bval.numpy())
    assert chk.keys() == sd.keys() and all(torch.equal(chk[k], sd[k]) for k in sd)
    # the oracle on the same weights reproduces the reference (the oracle is what the test runs beside the HIP model)
    ref, orc = ctor(), O.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16)
    for m in (ref, orc):
        m.load_state_dict(sd)
        prep(m)
    with torch.no_grad():
        MG.assert_close(orc(img)[0], ref(img)[0], 1e-4, "logits: oracle vs reference")
    MG.save(name, seed=seed, shape=torch.tensor(shape), beta_idx=bidx, beta_val=bval, **proof)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", help="records to mint (default: all)")
    ap.add_argument("--out", default=MG.OUT, help="output directory (default: tests/golden)")
    args = ap.parse_args()
    unknown = set(args.names) - {r[0] for r in RECORDS}
    if unknown:
        raise SystemExit("unknown record(s): %s" % ", ".join(sorted(unknown)))
    MG.OUT = args.out
    os.makedirs(MG.OUT, exist_ok=True)
    torch.set_num_threads(8)
    MG.install_shims()
    sys.path.insert(0, os.path.join(MG.REF, "DeepLabV3Plus-Pytorch"))
    import network as R  # the reference package

    for name, seed, shape in RECORDS:
        if not args.names or name in args.names:
            mint(R, name, seed, shape)


if __name__ == "__main__":
    main()
