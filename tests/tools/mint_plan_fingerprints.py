"""Mints tests/golden/plan_fingerprints.json: what every kind of plan launches, as a fingerprint of its op lists.

A plan builds on CPU tensors with the built library and launches nothing (store.bind(cpu), then plan_cls(engine, B, H, W, dtype,
training)), so the complete launch list of a plan -- every entry point, every argument, every descriptor field, the weight
preparation work and the replay bookkeeping -- can be pinned without a GPU.  The golden is minted from the code BEFORE a change of
the engine and must not move under a refactor; tests/test_plan_fingerprint.py rebuilds every case and compares.

Canonical form: one pointer map for the whole walk (null = 0, any other address numbered in order of first appearance: allocator
addresses go, the aliasing structure stays).  fwd, then bwd: each op by entry-point name ("py" for a host step), each argument by
its declared argtype; descriptors passed by reference field by field.  Then prep / prep_h2 / prep_gather and the bookkeeping the
replay reads.

    python tests/tools/mint_plan_fingerprints.py          # rewrites the golden
"""
import contextlib
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "tests")]
import helpers as H  # noqa: E402,F401  (puts the repo root and the package dir on sys.path)
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "plan_fingerprints.json")

PRODUCTS = {"exact": 0, "bf16x3": 1, "f16x2": 2}
# the switches of tests/test_gpu_model.py::PLAN_SWITCHES that act when a plan is BUILT and change an f16x2 plan (DML_GROUP_WGRAD
# groups bf16 weight gradients only: its case is a bf16 one; DML_PREP_OVERLAP / DML_OVERLAP_WGRAD / DML_NATIVE_PLAN act at replay)
BUILD_SWITCHES = ["DML_H2_DIRECT", "DML_FUSE_RES_GRAD", "DML_RES_PLANES", "DML_FUSE_BN_REDUCE", "DML_FUSE_BOUND", "DML_S2_CLASSES",
                  "DML_DS_GRAD_FROM_DZ", "DML_BNR_INC", "DML_CAT_PLANES", "DML_STEM_S2D"]


def _case(name, model, mode, shape, training=True, env=None, predict_heads=None, default=None):
    """mode: "bf16" or an fp32 product mode; default: the case this one must differ from (a switch case)"""
    return dict(name=name, model=model, mode=mode, shape=shape, training=training, env=env or {}, predict_heads=predict_heads,
                default=default)


def cases():
    out = []
    for B, Hh, Ww in ((2, 64, 64), (2, 128, 128), (1, 65, 97)):
        for mode in ("bf16", "exact", "bf16x3", "f16x2"):
            out.append(_case("train_%dx%dx%d_%s" % (B, Hh, Ww, mode), "deeplab16", mode, (B, Hh, Ww)))
    for B, Hh, Ww in ((1, 128, 256), (1, 65, 97)):
        for mode in ("bf16", "f16x2"):
            out.append(_case("infer_%dx%dx%d_%s" % (B, Hh, Ww, mode), "deeplab16", mode, (B, Hh, Ww), training=False))
    for mode in ("f16x2", "bf16"):
        out.append(_case("twohead_train_2x96x96_%s" % mode, "twohead", mode, (2, 96, 96)))
    out.append(_case("twohead_predict2_2x96x96_f16x2", "twohead", "f16x2", (2, 96, 96), training=False, predict_heads=2))
    out.append(_case("c21_os8_frozen_bn_train_2x65x97_f16x2", "deeplab21_os8_frozen", "f16x2", (2, 65, 97)))
    dflt = "train_2x128x128_f16x2"
    for sw in BUILD_SWITCHES:
        out.append(_case("train_2x128x128_f16x2_%s=0" % sw, "deeplab16", "f16x2", (2, 128, 128), env={sw: "0"}, default=dflt))
    out.append(_case("train_2x128x128_f16x2_all=0", "deeplab16", "f16x2", (2, 128, 128), env={sw: "0" for sw in BUILD_SWITCHES + ["DML_GROUP_WGRAD"]},
                     default=dflt))
    for sw, v in (("DML_FUSE_STEM", "0"), ("DML_FUSE_HEAD_DGRAD", "0"), ("DML_W_TILED", "0"), ("DML_WS_MIN_TILES", "1")):
        # (DML_W_TILED acts on bf16 weight copies: its case and its default are the bf16 plan)
        mode = "bf16" if sw == "DML_W_TILED" else "f16x2"
        out.append(_case("train_2x128x128_%s_%s=%s" % (mode, sw, v), "deeplab16", mode, (2, 128, 128), env={sw: v},
                         default="train_2x128x128_%s" % mode))
    for sw, v in (("DML_GRAD_STAGE32", "1"), ("DML_GROUP_WGRAD", "0")):
        out.append(_case("train_2x128x128_bf16_%s=%s" % (sw, v), "deeplab16", "bf16", (2, 128, 128), env={sw: v},
                         default="train_2x128x128_bf16"))
    for mode in ("bf16", "f16x2"):
        out.append(_case("ppm_infer_1x97x131_%s" % mode, "ppm", mode, (1, 97, 131), training=False))
    return out


_MODELS = {}


def _model(kind):
    """one model per kind for the whole run (weights do not matter); bound to the CPU once"""
    if kind not in _MODELS:
        torch.manual_seed(0)
        if kind == "ppm":
            from models import models
            enc = models.ModelBuilder.build_encoder("resnet50dilated", fc_dim=2048)
            dec = models.ModelBuilder.build_decoder("ppm_deepsup_embedding", fc_dim=2048, num_class=13, use_softmax=True)
            m = models.SegmentationModuleOOD(enc, dec, None)
        else:
            import network
            if kind == "twohead":
                m = network.deeplabv3plus_embedding_self_distillation_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
            elif kind == "deeplab21_os8_frozen":
                m = network.deeplabv3plus_embedding_resnet101(num_classes=21, output_stride=8, pretrained_backbone=False)
            else:
                m = network.deeplabv3plus_embedding_resnet101(num_classes=16, output_stride=16, pretrained_backbone=False)
        m._engine.store.bind(torch.device("cpu"))
        _MODELS[kind] = m
    return _MODELS[kind]


@contextlib.contextmanager
def _switches(env):
    """the process's DML_* switches replaced by `env` (DML_LIB_PATH, which selects the library, stays)"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("DML_") and k != "DML_LIB_PATH"}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def build_plan(case):
    m = _model(case["model"])
    m.train(case["training"])
    if case["model"] == "deeplab21_os8_frozen":
        m.backbone.layer1[0].bn1.eval()
    eng = m._engine
    eng.f32_split = 0 if case["mode"] == "bf16" else PRODUCTS[case["mode"]]
    dtype = torch.bfloat16 if case["mode"] == "bf16" else torch.float32
    B, Hh, Ww = case["shape"]
    with _switches(case["env"]):
        if case["predict_heads"] is not None:
            return eng.plan_cls(eng, B, Hh, Ww, dtype, case["training"], predict_heads=case["predict_heads"])
        return eng.plan_cls(eng, B, Hh, Ww, dtype, case["training"])


class _Canon:
    def __init__(self):
        self.ptrs = {}

    def ptr(self, v):
        if isinstance(v, C.c_void_p):
            v = v.value
        if not v:
            return 0
        return self.ptrs.setdefault(int(v), len(self.ptrs) + 1)

    def struct(self, st):
        out = [type(st).__name__]
        for f, t, *_ in st._fields_:
            v = getattr(st, f)
            if t is C.c_void_p:
                out.append(self.ptr(v))
            elif isinstance(v, C.Array):
                out.append(tuple(v))
            else:
                out.append(v)
        return out

    def arg(self, v, ctype):
        obj = getattr(v, "_obj", None)
        if isinstance(obj, C.Structure):                 # byref(descriptor)
            return self.struct(obj)
        if obj is not None:                              # byref(c_int): an out-parameter another op reads
            return ["box", self.ptr(C.addressof(obj)), obj.value]
        if isinstance(v, C._SimpleCData):                # a boxed c_int passed by value
            return ["box", self.ptr(C.addressof(v)), v.value]
        if ctype is C.c_void_p:
            return ["p", self.ptr(v)]
        return v

    def ops(self, ops):
        out = []
        for fn, args in ops:
            name, types = getattr(fn, "__name__", None), getattr(fn, "argtypes", None)
            if name is None or types is None or not name.startswith("dml_"):
                out.append(["py"])
                continue
            rec = [name] + [self.arg(v, t) for v, t in zip(args, types)]
            if name == "dml_conv_wgrad_group":
                rec.append([self.struct(d) for d in args.meta])
            out.append(rec)
        return out

    def rows(self, rows, pointer_positions):
        return [[self.ptr(v) if k in pointer_positions else v for k, v in enumerate(r)] for r in rows]


def _nonpointer_fields(descs):
    return [[getattr(d, f) for f, t, *_ in d._fields_ if t is not C.c_void_p] for d in descs]


def fingerprint(plan):
    from dmlnet import _lib
    c = _Canon()
    fwd, bwd = c.ops(plan.fwd), c.ops(plan.bwd)
    prep = c.rows(plan.prep, (0, 1, 2))
    prep_h2 = c.rows(plan.prep_h2, (0, 4, 8))
    prep_gather = c.rows(plan.prep_gather, (0, 1))
    where = {id(args): ("fwd", i) for i, (_, args) in enumerate(plan.fwd)}
    where.update({id(args): ("bwd", i) for i, (_, args) in enumerate(plan.bwd)})
    cat = getattr(plan, "cat_bound_table", None)
    cat_tab = []
    if cat is not None:
        raw = bytes(cat.cpu().numpy().tobytes())
        n = len(raw) // C.sizeof(_lib.H2BoundDesc)
        cat_tab = _nonpointer_fields((_lib.H2BoundDesc * n).from_buffer_copy(raw))
    book = dict(
        side=sorted(plan.side.items()), param_last_op=sorted(plan.param_last_op.items()), prep_cut=getattr(plan, "prep_cut", None),
        fwd_forks=getattr(plan, "fwd_forks", None), head_bwd_range=sorted(getattr(plan, "head_bwd_range", {}).items()),
        backbone_bwd_range=getattr(plan, "backbone_bwd_range", None), to_backbone_ops=getattr(plan, "to_backbone_ops", None),
        momentum_slots=[list(where[id(args)]) + [idx] for args, idx, _ in plan.momentum_slots],
        units=len(plan.units), drop_units=len(plan.drop_units),
        bn_eval=_nonpointer_fields(getattr(plan, "bn_eval", [])), h2_bound=_nonpointer_fields(getattr(plan, "h2_bound_tab", [])),
        cat_bound=cat_tab)
    canon = dict(fwd=fwd, bwd=bwd, prep=prep, prep_h2=prep_h2, prep_gather=prep_gather, book=book)
    text = json.dumps(canon, sort_keys=True, separators=(",", ":"), default=list)
    launches = {}
    for op in fwd + bwd:
        launches[op[0]] = launches.get(op[0], 0) + 1
    return dict(counts=dict(fwd=len(fwd), bwd=len(bwd), prep=len(prep), prep_h2=len(prep_h2), prep_gather=len(prep_gather)),
                launches=dict(sorted(launches.items())), bytes=int(plan.bytes), sha256=hashlib.sha256(text.encode()).hexdigest())


def mint():
    return {case["name"]: fingerprint(build_plan(case)) for case in cases()}


if __name__ == "__main__":
    out = mint()
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %d cases to %s" % (len(out), GOLDEN))
