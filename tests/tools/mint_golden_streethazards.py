"""Mint tests/golden/g15_streethazards.npz from the REFERENCE's own evaluation dataset (authoring container only).

anomaly/dataset.py of the reference is loaded by file path and its ValDataset run unchanged on a small synthetic
StreetHazards-layout tree (odd frame sizes; imgSizes / imgMaxSize overridden small so that the scales cover both up- and
down-scaling).  It needs torchvision.transforms.Normalize, which is not installed here, so a shim forwards it exactly as
torchvision does (as_tensor(mean / std, dtype) then sub_ / div_).  Outputs are data only: the source frames and
annotations, the options, and the tensors ValDataset returned.
"""
import importlib.util, json, os, sys, tempfile, types
import numpy as np
import torch
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference/anomaly/dataset.py"


class Normalize:
    def __init__(self, mean, std, inplace=False):
        self.mean, self.std = mean, std

    def __call__(self, t):
        t = t.clone()
        m = torch.as_tensor(self.mean, dtype=t.dtype, device=t.device)
        s = torch.as_tensor(self.std, dtype=t.dtype, device=t.device)
        return t.sub_(m[:, None, None]).div_(s[:, None, None])


tv = types.ModuleType("torchvision")
tvt = types.ModuleType("torchvision.transforms")
tvt.Normalize = Normalize
tv.transforms = tvt
sys.modules.update({"torchvision": tv, "torchvision.transforms": tvt})
sys.dont_write_bytecode = True
spec = importlib.util.spec_from_file_location("ref_anomaly_dataset", REF)
ds = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ds)

FRAMES = [(37, 53), (61, 45), (29, 70), (48, 48)]       # (h, w)
IMG_SIZES, IMG_MAX_SIZE, PADDING = (20, 33, 52, 90), 110, 8


def main():
    rs = np.random.RandomState(15)
    root = tempfile.mkdtemp()
    recs, imgs, segs = [], [], []
    for i, (h, w) in enumerate(FRAMES):
        # smooth content plus noise: the interpolation sees both gradients and edges
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([(yy * 5 + xx * 3) % 256, (xx * 7) % 256, (yy * 11 + 40) % 256], -1)
        img = np.clip(base + rs.randint(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8)
        seg = rs.randint(0, 15, (h, w)).astype(np.uint8)          # 0 (-> -1) .. 14 (-> 13, the anomaly class)
        os.makedirs(os.path.join(root, "images"), exist_ok=True)
        os.makedirs(os.path.join(root, "annotations"), exist_ok=True)
        Image.fromarray(img).save(os.path.join(root, "images", "%d.png" % i))
        Image.fromarray(seg, mode="L").save(os.path.join(root, "annotations", "%d.png" % i))
        recs.append({"fpath_img": "images/%d.png" % i, "fpath_segm": "annotations/%d.png" % i, "height": h, "width": w})
        imgs.append(img)
        segs.append(seg)
    odgt = os.path.join(root, "test.odgt")
    with open(odgt, "w") as f:
        f.write(json.dumps(recs) + "\n")
    opt = types.SimpleNamespace(imgSizes=IMG_SIZES, imgMaxSize=IMG_MAX_SIZE, padding_constant=PADDING)
    dset = ds.ValDataset(root, odgt, opt)
    out = {"img_sizes": np.array(IMG_SIZES), "img_max_size": IMG_MAX_SIZE, "padding_constant": PADDING,
           "n_frames": len(FRAMES)}
    for i in range(len(FRAMES)):
        item = dset[i]
        out["img_%d" % i] = imgs[i]
        out["segm_%d" % i] = segs[i]
        out["seg_label_%d" % i] = item["seg_label"][0].numpy()
        for k, t in enumerate(item["img_data"]):
            out["out_%d_%d" % (i, k)] = t[0].numpy()
        print(i, imgs[i].shape, [tuple(t.shape[2:]) for t in item["img_data"]])
    path = os.path.join(ROOT, "tests", "golden", "g15_streethazards.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
