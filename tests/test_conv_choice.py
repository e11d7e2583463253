"""The kernel choice of the convolution library (csrc/conv_choice.h) against what the library launched before the choice was
separated from the launch: tests/golden/conv_choice_cases.json.gz (2.9 MB of JSON, gzip-compressed) holds descriptors -- every distinct one of the real plans plus
hand-written edge cases around each threshold and one per error return -- with the kernel, grid, tiling and reduce launches the
earlier host code issued for them (minted from that code, never from the header: tests/tools/mint_golden.py).  No GPU: the header is
pure host code, tests/tools/conv_choice_dump.cpp prints its answers."""
import gzip
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = os.path.join(ROOT, "tests", "golden", "conv_choice_cases.json.gz")
DUMP_SRC = os.path.join(ROOT, "tests", "tools", "conv_choice_dump.cpp")

# field order of DmlConvDesc / DmlWgradDesc (include/dmlnet_hip.h); "p": a pointer
CONV_FIELDS = [("x", "p"), ("w", "p"), ("y", "p"), ("bias", "p"), ("stats", "p")] + [(n, "i") for n in (
    "B", "Hi", "Wi", "C", "ldx", "Ho", "Wo", "N", "ldy", "R", "S", "stride", "dil", "pad", "dtype", "y_f32", "accum", "mode")] + [
    ("bnr_y", "p"), ("bnr_mask", "p"), ("bnr_mean", "p"), ("bnr_invstd", "p"), ("bnr_partials", "p"), ("bnr_ldy", "i"), ("bnr_relu", "i"),
    ("post_scale", "p"), ("post_shift", "p"), ("post_mean", "p"), ("post_res", "p"), ("post_ldres", "i"), ("post_relu", "i"),
    ("tail_ws", "p"), ("tail_ws_elems", "i"), ("tail_counters", "p"), ("tail_counters_len", "i"), ("tail_reserved", "i"),
    ("res_dz", "p"), ("res_mask", "p"), ("res_ld", "i"), ("res_reserved", "i"),
    ("acc32", "p"), ("acc32_ld", "i"), ("f32_split", "i"), ("w_tiled", "i"), ("ws_min_tiles", "i"),
    ("x_planes", "p"), ("w_planes", "p"), ("x_unscale", "p"), ("w_unscale", "p"), ("x_plane_stride", "i"), ("w_plane_stride", "i"),
    ("bnr_gmax", "p"), ("sub_grid", "i"), ("sub_y", "i"), ("sub_x", "i"), ("pad_w_set", "i"), ("pad_w", "i"), ("bnr_inc", "i")]
WGRAD_FIELDS = [("x", "p"), ("dy", "p"), ("dw", "p")] + [(n, "i") for n in (
    "B", "Hi", "Wi", "C", "ldx", "Ho", "Wo", "N", "ldy", "R", "S", "stride", "dil", "pad", "dtype", "splitk", "Cm")] + [
    ("ws", "p"), ("ws_elems", "i"), ("f32_split", "i"), ("reserved", "i"),
    ("x_planes", "p"), ("dy_planes", "p"), ("x_unscale", "p"), ("dy_unscale", "p"), ("x_plane_stride", "i"), ("dy_plane_stride", "i")]


# what a field of a table entry is when the entry leaves it out (everything else: 0); "=F": the value of field F
DEFAULTS = {"x": 16, "w": 16, "y": 16, "dy": 16, "dw": 16, "stride": 1, "dil": 1, "ldx": "=C", "ldy": "=N", "S": "=R", "Wi": "=Hi", "Wo": "=Ho"}


def expand(d, fields):
    """a table entry with its defaults filled in"""
    names = {n for n, _ in fields}
    out = dict(d)
    for n, v in DEFAULTS.items():
        if n in names and n not in out and not isinstance(v, str):
            out[n] = v
    for n, v in DEFAULTS.items():
        if n in names and n not in out and isinstance(v, str):
            out[n] = out.get(v[1:], 0)
    return out


def _tokens(d, fields, slot0=0):
    """A descriptor of the table as the dump program reads it.  The table keeps of a pointer what the choice may look at: 0 = null,
    16 + its low four address bits otherwise, and whether x (dy) IS x_planes (dy_planes); here every pointer gets an address of
    its own with those bits."""
    addr = {}
    d = expand(d, fields)
    for i, (n, t) in enumerate(fields):
        if t == "p":
            v = int(d.get(n, 0))
            addr[n] = 0 if v == 0 else (0x10000000 + (slot0 + i) * 0x100000 + (v - 16))
    if d.get("x_is_planes"):
        addr["x"] = addr["x_planes"]
    if d.get("dy_is_planes"):
        addr["dy"] = addr["dy_planes"]
    return [str(addr[n]) if t == "p" else str(int(d.get(n, 0))) for n, t in fields]


def variants(c):
    """(id, switches, expected line) of a case: a forward / data-gradient descriptor once per switch setting listed for it
    ("pick": which of the case's distinct expected lines that setting gives)"""
    if c["kind"] != "C":
        return [(c["id"] + ".0", None, c["expect"][0])]
    return [("%s.%d" % (c["id"], i), sw, c["expect"][c["pick"][i]]) for i, sw in enumerate(c["sw"])]


def case_line(c, vid, sw):
    if c["kind"] == "C":
        toks = [vid, "C"] + [str(int(v)) for v in sw] + _tokens(c["d"], CONV_FIELDS)
    elif c["kind"] == "W":
        toks = [vid, "W"] + _tokens(c["d"], WGRAD_FIELDS)
    else:
        ws = 0 if not c["ws"] else 0x70000000 + (c["ws"] - 16)
        toks = [vid, "G", str(len(c["jobs"])), str(ws), str(int(c["ws_elems"]))]
        for j, d in enumerate(c["jobs"]):
            toks += _tokens(d, WGRAD_FIELDS, slot0=40 * (j + 1))
    return " ".join(toks) + "\n"


def _fields(line):
    return dict(t.split("=", 1) for t in line.split())


def _host_compiler():
    """the clang++ that the Makefile's hipcc drives; hipcc itself on a C++ source otherwise"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    for rel in ("../lib/llvm/bin/clang++", "../llvm/bin/clang++"):
        p = os.path.normpath(os.path.join(os.path.dirname(os.path.realpath(hipcc)), rel))
        if os.path.exists(p):
            return [p]
    return [hipcc, "-x", "c++"]


@pytest.fixture(scope="module")
def golden():
    with gzip.open(CASES, "rt") as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def table(golden):
    return golden["cases"]


@pytest.fixture(scope="module")
def chosen(table, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("conv_choice") / "conv_choice_dump")
    r = subprocess.run(_host_compiler() + ["-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", DUMP_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], input="".join(case_line(c, vid, sw) for c in table for vid, sw, _ in variants(c)), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    out = {}
    for ln in r.stdout.splitlines():
        i, _, rest = ln.partition(" ")
        out[i] = rest
    return out


def test_header_is_plain_cxx17():
    """conv_choice.h includes only the C ABI header and the standard library: it compiles with plain g++ -std=c++17"""
    hdr = os.path.join(ROOT, "open-world-semantic-segmentation_amd", "csrc", "conv_choice.h")
    src = open(hdr).read()
    incs = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert incs == ["<cstdint>", '"../../include/dmlnet_hip.h"'], incs
    assert "__device__" not in src and "__global__" not in src and "getenv" not in src.replace("conv_igemm.hip", "")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-x", "c++", "-include", hdr, os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_every_case_chooses_what_the_library_launched(table, chosen):
    assert len(table) > 400 and len({c["id"] for c in table}) == len(table)
    bad = []
    n = 0
    for c in table:
        assert len(c["expect"]) == 1 if c["kind"] != "C" else len(c["sw"]) == len(c["pick"]) >= 1
        for vid, sw, expect in variants(c):
            n += 1
            assert vid in chosen, "no answer for case %s" % vid
            want, got = _fields(expect), _fields(chosen[vid])
            if want != got:
                diff = {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}
                bad.append("%s %s %s: (expected, chosen) %s" % (vid, c["src"], sw, diff))
    assert n == len(chosen) > 1000
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), n, "\n".join(bad[:20]))


def _instantiations():
    conv = set()
    for t in ("bf16", "f32"):
        for bn in (128, 64, 32):
            for al in (0, 1):
                for mode in (0, 1):
                    conv.add("conv_igemm_kernel<%s,%d,%d,%d>" % (t, bn, al, mode))
    for mode in (0, 1, 2):
        conv |= {"conv_igemm_dma_kernel<128,%d,3,2,256,128>" % mode, "conv_igemm_dma_kernel<128,%d,3,3,128,64>" % mode,
                 "conv_igemm_dma_kernel<64,%d,3,3,128,64>" % mode, "conv_ws_kernel<1,4,%d,3,1,9,0>" % mode, "conv_ws_kernel<2,2,%d,3,1,9,0>" % mode}
    conv |= {"conv_ws_kernel<1,4,0,3,2,3,0>", "conv_ws_kernel<4,1,0,3,2,3,0>", "conv_ws_kernel<1,4,0,3,2,9,0>", "conv_ws_kernel<2,2,0,3,2,9,0>"}
    for epi in range(4):
        conv |= {"conv_ws_kernel<4,1,1,3,2,3,%d>" % epi, "conv_ws_kernel<1,4,1,3,2,9,%d>" % epi, "conv_ws_kernel<2,2,1,3,2,9,%d>" % epi}
    for mode in (0, 1):
        conv |= {"conv_igemm_x3_kernel<128,%d>" % mode, "conv_igemm_x3_kernel<64,%d>" % mode}
    wgrad = {"conv_wgrad_big_kernel<2>", "conv_wgrad_ws_kernel<0>", "conv_wgrad_ws_kernel<1>", "conv_wgrad_h2_kernel<0>", "conv_wgrad_h2_kernel<1>",
             "conv_wgrad_n64_kernel", "conv_wgrad_x3_kernel<0>", "conv_wgrad_x3_kernel<1>", "conv_wgrad_kernel<bf16>", "conv_wgrad_kernel<f32>"}
    return conv, wgrad


def test_table_covers_every_instantiation_and_error_code(table):
    """every kernel instantiation dml_conv_igemm / dml_conv_wgrad / dml_conv_wgrad_group can launch and every error code of each entry
    point appear in the table (the expected side: what the library launched), and nothing outside the list"""
    conv, wgrad = _instantiations()
    seen = {"C": set(), "W": set(), "G": set()}
    codes = {"C": set(), "W": set(), "G": set()}
    reduces = set()
    rows = set()
    for c in table:
        for _, _, expect in variants(c):
            f = _fields(expect)
            codes[c["kind"]].add(int(f["rc"]))
            if "k" in f:
                seen[c["kind"]].add(f["k"])
            if c["kind"] == "W" and "k" in f:
                reduces.add(sum(1 for k in f if k.startswith("reduce")))
            if c["kind"] == "C":
                rows.add(f["rows"])
    assert seen["C"] == conv, (sorted(conv - seen["C"]), sorted(seen["C"] - conv))
    assert seen["W"] == wgrad, (sorted(wgrad - seen["W"]), sorted(seen["W"] - wgrad))
    assert seen["G"] == {"conv_wgrad_group_kernel<2>"}
    assert codes["C"] == {0, -1, -2, -3} and codes["W"] == {0, -1, -2, -3} and codes["G"] == {0, -1, -3}, codes
    assert reduces == {0, 1, 2}      # atomics, one fold launch, chunked fold in two launches
    assert rows == {"64", "48", "144"}, rows


SMALL = ["2x64x64", "2x128x128", "4x96x128", "1x256x256", "1x65x97", "3x50x34", "2x128x192", "2x97x129", "2x64x80", "2x96x96", "2x64x96"]
PLANS = ["train_16x768x768_" + dt for dt in ("bf16", "f16x2", "f32x3", "f32")] + [
    "fwd_8x768x768_f16x2", "fwd_8x768x768_bf16", "infer_1x1024x2048_f16x2", "infer_1x1024x2048_bf16"] + [
    "train_%s_%s" % (sz, dt) for sz in SMALL for dt in ("bf16", "f16x2", "f32x3", "f32")]


def test_table_holds_the_real_plans(golden, table):
    """descriptors of the plans the benchmark and the suite build (deduplicated: a case names the first plan it came from; "plans"
    lists every plan that went in, with its descriptor counts)."""
    for p in PLANS:
        assert p in golden["plans"] and golden["plans"][p][0] > 50, p
    for p in PLANS:
        assert not p.startswith("train") or golden["plans"][p][1] > 100, p
    assert golden["plans"]["train_16x768x768_bf16"][2] > 20      # grouped weight-gradient launches
    kinds = {(c["kind"], c["src"].split(":")[0]) for c in table}
    assert {("C", "plan"), ("W", "plan"), ("G", "plan"), ("C", "edge"), ("W", "edge"), ("G", "edge"), ("C", "err"), ("W", "err"), ("G", "err")} <= kinds
    # the switches: every setting the suite and the documentation use
    sws = {tuple(sw) for c in table if c["kind"] == "C" for sw in c["sw"]}
    assert {(0, 1, 0), (1, 1, 0), (0, 0, 0), (0, 2, 0), (0, 2304, 0), (0, 1, 1)} <= sws
