"""The split-3 GEMM cases (tests/gemm_split3_cases.py) planned without a GPU: every case reaches the instantiation it names, the table
covers every split-3 instantiation of CVLM_GEMM_KERNELS (csrc/gemm_plan.h) in every form the planner admits on it, and which pair of
kernels each parametrisation of the relation tests of tests/test_ops_gpu.py compares.  The mx kernels (CVLM_GEMM_MX_KERNELS) are out
of scope here: tests/test_gemm_mx_gpu.py holds them."""
import collections
import os
import re

import pytest
import torch

import gemm_split1_cases as S1
import gemm_split3_cases as S3
from camouflaged_vlm_amd import hip

PLAN_H = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "csrc", "gemm_plan.h")
CUS = 256                                                              # the CU count the CPU plans assume (an MI355X)
KEY_OF = {k.name: k.key for k in S3.KERNELS.values()}


def _set_env(monkeypatch, env):
    for name in [n for n in os.environ if n.startswith("CVLM_GEMM_") and n != "CVLM_GEMM_VARIANT_LIVE"]:
        monkeypatch.delenv(name)
    for name, value in env.items():
        monkeypatch.setenv(name, value)


@pytest.fixture(scope="module")
def ws():
    return torch.zeros(hip.gemm_workspace_bytes(), dtype=torch.uint8)   # never touched: the planner asks only whether it is there


def split3_kernels_of_the_library():
    """the split-3 entries of CVLM_GEMM_KERNELS as a demangler prints them, CVLM_X_IL expanded"""
    with open(PLAN_H) as f:
        text = f.read()
    body = text[text.index("#define CVLM_GEMM_KERNELS(X)"):text.index("#define CVLM_X_IL(")]
    dflt = ["", "", "", "", "", "0", "4", "false", "-1", "false", "false", "false", "false", "false"]
    names = []
    for il, m in re.findall(r"\b(CVLM_X_IL\(X,|X\()([^()]*)\)", body):
        args = [a.strip() for a in m.split(",")]
        for tail in ((["true", "false"], ["true", "true"]) if il.startswith("CVLM_X_IL") else ([],)):
            full = args + tail
            names.append("gemm_nt_kernel<" + ", ".join(full + dflt[len(full):]) + ">")
    assert len(set(names)) == len(names)
    return {n for n in names if n.startswith("gemm_nt_kernel<3,")}


def test_every_case_reaches_the_kernel_it_names(monkeypatch, ws):
    """Under the case's environment the planner gives one launch of the named instantiation, with the K-parts the case names, for the
    very arguments the GPU test passes to hip.gemm; the plain launch a head-major case is compared with plans the same way.  Over the
    table: exactly the split-3 entries of CVLM_GEMM_KERNELS, so a new instantiation without a case fails here."""
    assert os.environ.get("CVLM_GEMM_VARIANT_LIVE") == "1", "tests/conftest.py: the knobs are re-read per call"
    assert len({c.id for c in S3.CASES}) == len(S3.CASES)
    reached = set()
    for c in S3.CASES + S3.EXTRA_CASES:                            # the parity launches of the GPU file as well
        _set_env(monkeypatch, c.env)
        L = S3.launch(c, hip, "cpu", workspace=ws, cus=CUS)
        plan = hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, cus=CUS, **L.kw)
        want = S3.expected_plan(c, L.M, L.N)
        assert len(plan) == 1 and {k: plan[0][k] for k in want} == want, (c.id, plan, want)
        if c.k.persist:
            assert plan[0]["total_blocks"] > CUS and plan[0]["grid_x"] == CUS, (c.id, plan)
        reached.add(plan[0]["kernel"])
        if c.form == "head_major":
            kw = {k: v for k, v in L.kw.items() if k not in ("head_major", "head_major_nolo")}
            plain = hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, cus=CUS, **kw)
            assert len(plain) == 1 and {k: plain[0][k] for k in want} == want, (c.id, plain)
        if c.k.il:                                                  # the planar launch an image case is compared with
            p = S3.planar_twin(c)
            _set_env(monkeypatch, p.env)
            P = S3.launch(p, hip, "cpu", workspace=ws, cus=CUS)
            plan = hip.gemm_plan(P.A, P.W, P.M, P.N, P.K, cus=CUS, **P.kw)
            want = S3.expected_plan(p, P.M, P.N)
            assert len(plan) == 1 and {k: plan[0][k] for k in want} == want, (p.id, plan, want)
    library = split3_kernels_of_the_library()
    assert len(library) == 42 and reached == library == {k.name for k in S3.KERNELS.values()}, (reached ^ library)


def _edge_classes(k, shp):
    """which of the edges the issue names the (M, N, K) shapes of kernel k cover"""
    (tm, tn), r = k.tile, k.ring
    got = set()
    for M, N, K in shp:
        nk = K // 32
        if M < tm and N < tn:
            got.add("one ragged tile")
        if M % tm == 1 and N % tn in (1, 8):
            got.add("one past the edge")
        if N % 64 == 8:
            got.add("8-column last piece")
        got |= {name for name, v in (("nk=1", 1), ("nk=R-1", r - 1), ("nk=R", r), ("nk=R+1", r + 1)) if nk == v}
        if nk >= 40:
            got.add("long K")
    return got


ALL_EDGES = {"one ragged tile", "one past the edge", "8-column last piece", "nk=1", "nk=R-1", "nk=R", "nk=R+1", "long K"}


def test_table_has_every_form_and_edge_on_every_kernel():
    """Per kernel family the set of forms and the edge classes of its shapes: a form or an edge dropped from the table shows here."""
    by = collections.defaultdict(list)
    for c in S3.CASES:
        by[c.kernel].append(c)
    forms = lambda key: {c.form for c in by[key]}
    shapes3 = lambda key, *fs: {c.shape for c in by[key] if c.form in (fs or ("product", "plain", "ln_fold", "h2_residual")) and not c.tail}
    every = set(S3.FORMS_GENERIC)
    for key in ("r2", "r3", "r4", "r5", "w64", "w128", "k2"):
        k = S3.KERNELS[key]
        assert forms(key) == (every if key in ("r2", "k2") else every - {"batched"}), key      # a batch is not one3: no ring kernel
        assert _edge_classes(k, shapes3(key)) == ALL_EDGES, key
        for shape in S3.shapes(k):
            plain = [c for c in by[key] if c.form == "plain" and c.shape == shape]
            assert {c.act for c in plain if c.layout == "tight"} == {0, 1, 2, 3} and {c.layout for c in plain} == set(S1.LAYOUTS), (key, shape)
        staged = {s for s in S3.shapes(k) if s[1] % 8 == 0}
        assert len(staged) == 3 and all(s[1] % 64 == 8 for s in staged)
        assert {(c.shape, c.act) for c in by[key] if c.form == "ln_fold"} == {(s, a) for s in staged for a in (0, 1, 2)}, key
        assert shapes3(key, "h2_residual") == staged, key
        assert {(c.shape, c.nolo) for c in by[key] if c.form == "head_major"} == {(s, n) for s in S1.HEAD_MAJOR_SHAPES for n in (0, 2, 5)}
    # the all-forms 256^2 kernel: what the staged path cannot store (the fold and the h2 residual exist on the staged path only)
    assert forms("g256") == every - {"ln_fold", "h2_residual"}
    assert _edge_classes(S3.KERNELS["g256"], shapes3("g256")) == ALL_EDGES - {"8-column last piece"}      # N % 8 == 0 goes to e0
    for shape in S3.G256_SHAPES:
        plain = [c for c in by["g256"] if c.form == "plain" and c.shape == shape]
        assert {c.act for c in plain if c.layout == "tight"} == {0, 1, 2, 3} and {c.layout for c in plain} == set(S1.LAYOUTS)
    # split-K: every one-problem form, parts 2 / 4 / 8, an uneven split; and on the image twins
    for key in ("sk_r2", "sk_r3", "sk_r4", "sk_w8"):
        assert forms(key) == every - {"batched"}, key
        assert {c.parts for c in by[key]} == {2, 4, 8}
        assert {c.parts for c in by[key] if c.form in ("ln_fold", "h2_residual")} == {4, 8}
        assert any((c.shape[2] // 32) % c.parts for c in by[key] if c.form == "plain")
    for key in ("sk_w8-w", "sk_w8-wa"):
        assert {c.parts for c in by[key]} == {2, 4, 8}, key
    # the epilogue-specialised 256^2 kernels, one-pass: their form at every edge, plus one case per count of tail parts
    want = {"e0": {"product", "plain", "head_major"}, "e1": {"ln_fold"}, "e2": {"h2_residual"}}
    for key, fs in want.items():
        assert forms(key) == fs, key
        assert _edge_classes(S3.KERNELS[key], shapes3(key)) == ALL_EDGES, key
        assert {c.parts for c in by[key] if c.tail} == {2, 3, 4}, key
    for shape in S3.EPI_SHAPES:
        plain = [c for c in by["e0"] if c.form == "plain" and c.shape == shape]
        assert {c.act for c in plain if c.layout == "tight" and c.outs == "both"} == {0, 1, 2, 3}
        assert {(c.layout, c.outs) for c in plain} == {("tight", "both"), ("padded", "both"), ("tight", "h2"), ("tight", "f32")}
        assert {c.act for c in by["e1"] if c.shape == shape} == {0, 1, 2}
    assert {(c.shape, c.nolo) for c in by["e0"] if c.form == "head_major"} == {(s, n) for s in S3.EPI_HEAD_MAJOR for n in (0, 2, 5)}
    # persistent: more tiles than CUs, nk = 1, R, R + 1
    for key, fs in (("p0", want["e0"]), ("p1", want["e1"]), ("p2", want["e2"])):
        assert forms(key) == fs, key
        assert {c.shape for c in by[key] if c.form != "head_major"} == {(S3.TALL, 264, kk) for kk in S3.TALL_K}, key
    assert {(c.layout, c.outs) for c in by["p0"] if c.form == "plain"} == {("tight", "both"), ("padded", "both"), ("tight", "h2"), ("tight", "f32")}
    assert {c.nolo for c in by["p0"] if c.form == "head_major"} == {0, 2, 5}
    assert {c.act for c in by["p1"]} == {0, 1, 2}
    # 192-row tiles: a last tile of one row, of 72 rows, long K (K < 512 never reaches it: gemm_split3_cases.py)
    assert forms("t192") == {"h2_residual"} and {c.shape for c in by["t192"]} == set(S3.T192_SHAPES)
    assert {s[0] % 192 for s in S3.T192_SHAPES} == {72, 1} and max(s[2] for s in S3.T192_SHAPES) >= 2048
    assert forms("conv") == {"conv"} and len(by["conv"]) == 3
    # image twins: the forms of the il_any block on each, an image output on the weight-and-activation twin
    for k in S3.KERNELS.values():
        if not k.il:
            continue
        fs = {"generic": {"plain", "ln_fold", "h2_residual", "head_major"}, "epi0": {"plain", "head_major"}, "epi1": {"ln_fold"},
              "epi2": {"h2_residual"}, "t192": {"h2_residual"}, "sk": {"plain", "ln_fold", "h2_residual"}}[k.kind]
        assert forms(k.key) == fs, k.key
        assert any(c.out_il for c in by[k.key]) == (k.il == "wa"), k.key
        if k.kind in ("epi0", "epi1", "epi2") and not k.persist:
            assert any(c.tail for c in by[k.key]), k.key


# ---------------------------------------------------------------------------------------------
# The relation tests of tests/test_ops_gpu.py planned with their own arguments.  The planner reads shapes, leading dimensions and which
# pointers are given; the tensors below are never dereferenced.

def _plan_keys(monkeypatch, env, M, N, K, form, ws=None, w_il=False, a_il=False, out_il=False, head_major=None):
    """kernels (keys of gemm_split3_cases.KERNELS) of the launches of one call in the form a relation test issues"""
    _set_env(monkeypatch, env)
    e = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype)
    h2 = lambda cols: hip.H2(e(2, 1, 8, dtype=torch.float16)) if not out_il else hip.H2IL(e(1, 2 * (cols + 64 - cols % 32), dtype=torch.float16))
    a = hip.H2IL(e(1, 2 * K, dtype=torch.float16)) if a_il else hip.H2(e(2, 1, 8, dtype=torch.float16))
    w = hip.H2(e(2, 1, 8, dtype=torch.float16))
    kw = dict(bias=e(8), workspace=ws)
    if w_il or a_il:
        kw.update(w_il=e(1, 2 * K, dtype=torch.float16))
    if form == "f32":
        kw.update(out_f32=e(8))
    elif form == "f32_h2":
        kw.update(out_f32=e(8), out_h2=h2(N))
    elif form == "f32_residual":
        kw.update(out_f32=e(8), residual=e(8))
    elif form == "h2":
        kw.update(out_h2=h2(N))
    elif form == "head_major":
        kw.update(out_h2=h2(N), head_major=head_major)
    elif form == "ln_fold":
        kw.update(out_h2=h2(N), act=1, ln_fold=(e(M, 2), e(8)))
    elif form == "h2_residual":
        o = h2(N)
        kw.update(out_h2=o, residual_h2=(o, 4.0), out_scale=0.25, row_stats=e(hip.stats_pieces(N), M, 2))
    else:
        raise ValueError(form)
    plan = hip.gemm_plan(a, w, M, N, K, cus=CUS, **kw)
    return tuple(KEY_OF[p["kernel"]] + (f"/tail{p['tail_split']}" if p["tail_split"] > 1 else "") + (f"/sk{p['sk_parts']}" if p["sk_parts"] > 1 else "")
                 for p in plan)


def _params(name):
    """the parametrisations of a test of tests/test_ops_gpu.py: the tables below speak of today's tests"""
    import test_ops_gpu
    marks = [m for m in getattr(test_ops_gpu, name).pytestmark if m.name == "parametrize"]
    assert len(marks) == 1
    return tuple(tuple(a) if isinstance(a, (tuple, list)) else a for a in marks[0].args[1])


PERSISTENT_EQUALS_PLAIN = {                                            # form -> (CVLM_GEMM_PERSIST=0, =1)
    "h2": (("e0",), ("p0",)),
    "f32_residual": (("e0",), ("p0",)),
    "head_major": (("e0",), ("p0",)),
    "ln_fold_gelu": (("e1",), ("p1",)),
    "h2_residual_stats": (("e2",), ("p2",)),
}


def test_relation_persistent_equals_plain(monkeypatch, ws):
    """test_gemm_persistent_equals_plain (VARIANT=7, TAIL=0, a workspace; 304 tiles, head-major 288, on 256 CUs):

        form                 PERSIST=0   PERSIST=1
        h2                   e0          p0
        f32_residual         e0          p0
        head_major           e0          p0
        ln_fold_gelu         e1          p1
        h2_residual_stats    e2          p2

    every parametrisation compares the one-pass kernel with the persistent one of the same epilogue form."""
    assert _params("test_gemm_persistent_equals_plain") == tuple(PERSISTENT_EQUALS_PLAIN)
    got = {}
    for form, mine in (("h2", "h2"), ("f32_residual", "f32_residual"), ("head_major", "head_major"), ("ln_fold_gelu", "ln_fold"),
                       ("h2_residual_stats", "h2_residual")):
        M, N, K, hm = (9 * 1024, 3 * 8 * 80, 96, (1024, 8, 80)) if form == "head_major" else (4648 + 8, 4096 - 8, 128, None)
        got[form] = tuple(_plan_keys(monkeypatch, {"CVLM_GEMM_TAIL": "0", "CVLM_GEMM_VARIANT": "7", "CVLM_GEMM_PERSIST": p}, M, N, K, mine,
                                     ws=ws, head_major=hm) for p in ("0", "1"))
    assert got == PERSISTENT_EQUALS_PLAIN, got
    assert all(a != b for a, b in got.values())


T192_PARAMS = ((9296, 1024, 256), (9296 - 100, 1024, 4096), (6000, 768, 128), (4104, 2056, 512))
T192_PAIRS = {                                                         # (M, N, K) -> (CVLM_GEMM_T192=0, =1)
    (9296, 1024, 256): (("k2",), ("k2",)),
    (9196, 1024, 4096): (("e2",), ("t192",)),
    (6000, 768, 128): (("k2",), ("k2",)),
    (4104, 2056, 512): (("e2",), ("t192",)),
}


def test_relation_192_row_tiles(monkeypatch, ws):
    """test_gemm_192_row_tiles_equal_256_row_tiles (VARIANT=0, a workspace, h2-residual form with row statistics):

        M x N x K              T192=0     T192=1
        9296 x 1024 x 256      256x128    256x128     the model prefers 256 x 128 tiles at K = 256: a kernel against itself
        9196 x 1024 x 4096     e2         t192
        6000 x 768 x 128       256x128    256x128     the same at K = 128
        4104 x 2056 x 512      e2         t192        added with this table: a last 192-row tile of 72 rows

    The 192-row kernel needs the model to prefer 256^2 tiles, i.e. 0.0685 K + 14 us <= 1.04 x two rounds of 256 x 128 tiles: K >= 512."""
    assert _params("test_gemm_192_row_tiles_equal_256_row_tiles") == T192_PARAMS
    got = {s: tuple(_plan_keys(monkeypatch, {"CVLM_GEMM_T192": f}, *s, "h2_residual", ws=ws) for f in ("0", "1")) for s in T192_PARAMS}
    assert got == T192_PAIRS, got
    assert sum(a != b for a, b in got.values()) >= 2


IL_WEIGHT_PARAMS = ((16640, 1280, 256, "7", False), (8192, 1280, 320, "7", True), (9296, 1024, 512, "0", True), (8200, 1160, 256, "2", True),
                    (4096, 5120, 256, "0", True), (581, 1024, 1024, "0", True), (581, 4096, 1024, "0", True), (581, 1024, 4096, "0", True))
IL_WEIGHT_KERNELS = {                                                  # -> planar kernels of the (plain f32, fold, h2-residual) launches
    (16640, 1280, 256): (("p0",), ("p1",), ("p2",)),
    (8192, 1280, 320): (("e0",), ("e1",), ("e2",)),
    (9296, 1024, 512): (("e0",), ("e1",), ("t192",)),
    (8200, 1160, 256): (("k2",), ("k2",), ("k2",)),
    (4096, 5120, 256): (("k2", "w128"), ("k2", "w128"), ("k2",)),       # the column split: 256 x 128 tiles, the rest on 128^2
    (581, 1024, 1024): (("w64",), ("w64",), ("w64",)),
    (581, 4096, 1024): (("w128",), ("w128",), ("w128",)),
    (581, 1024, 4096): (("sk_w8/sk4",), ("sk_w8/sk4",), ("sk_w8/sk4",)),
}


def _twin_of(keys, il):
    return tuple(k.split("/")[0] + "-" + il + ("/" + k.split("/")[1] if "/" in k else "") for k in keys)


def test_relation_interleaved_weights(monkeypatch, ws):
    """test_gemm_interleaved_weights_same_bits: each of its three launches (plain f32, LayerNorm fold, h2 residual) runs on kernel X
    without the image and on its weight-image twin X-w with it -- two different instantiations in every parametrisation:

        M x N x K (VARIANT)          plain          fold           h2 residual
        16640 x 1280 x 256 (7)       p0             p1             p2
        8192 x 1280 x 320 (7)        e0             e1             e2
        9296 x 1024 x 512 (0)        e0             e1             t192
        8200 x 1160 x 256 (2)        k2             k2             k2
        4096 x 5120 x 256 (0)        k2 + w128      k2 + w128      k2           (column split; the 256 x 128 kernel, not 256^2)
        581 x 1024 x 1024 (0)        w64            w64            w64
        581 x 4096 x 1024 (0)        w128           w128           w128
        581 x 1024 x 4096 (0)        sk_w8, 4 parts (all three)"""
    assert _params("test_gemm_interleaved_weights_same_bits") == IL_WEIGHT_PARAMS
    for M, N, K, variant, use_ws in IL_WEIGHT_PARAMS:
        for form, want in zip(("f32", "ln_fold", "h2_residual"), IL_WEIGHT_KERNELS[(M, N, K)]):
            got = [_plan_keys(monkeypatch, {"CVLM_GEMM_VARIANT": variant}, M, N, K, form, ws=ws if use_ws else None, w_il=il) for il in (False, True)]
            assert got == [want, _twin_of(want, "w")], (M, N, K, form, got)


IL_ACT_PARAMS = ((16640, 1280, 256, "7", False), (8192, 1280, 320, "7", True), (33000, 1280, 128, "0", True), (8200, 1160, 256, "2", True),
                 (4096, 3840, 256, "0", True), (4096, 5120, 256, "0", True), (4096, 1280, 1280, "0", True), (581, 1024, 1024, "0", True),
                 (581, 4096, 1024, "0", True), (581, 1024, 4096, "0", True))
IL_ACT_KERNELS = dict(IL_WEIGHT_KERNELS)
IL_ACT_KERNELS.pop((9296, 1024, 512))
IL_ACT_KERNELS.update({(33000, 1280, 128): (("k2",),) * 3, (4096, 3840, 256): (("k2",),) * 3, (4096, 1280, 1280): (("k2",),) * 3})


def test_relation_interleaved_activations(monkeypatch, ws):
    """test_gemm_interleaved_activations_same_bits: its planar reference launches pass the weight image, so each of the three forms
    compares the weight-image twin X-w with the weight-and-activation twin X-wa (image in, image out) -- two instantiations in every
    parametrisation.  X per form is that of the table above, and for the parametrisations this test has on its own:

        33000 x 1280 x 128 (0)       k2   (all three forms; its comment expects tail parts behind whole 256^2 tiles: with an
        4096 x 3840 x 256 (0)        k2    activation image the model compares 256^2 with 256 x 128 tiles only, and at these K the
        4096 x 1280 x 1280 (0)       k2    256 x 128 kernel wins each time)

    so no relation test runs chained K-parts on an image twin; tests/gemm_split3_cases.py has a tail case on each of e0 / e1 / e2 -w
    and -wa."""
    assert _params("test_gemm_interleaved_activations_same_bits") == IL_ACT_PARAMS
    for M, N, K, variant, use_ws in IL_ACT_PARAMS:
        for form, want in zip(("h2", "ln_fold", "h2_residual"), IL_ACT_KERNELS[(M, N, K)]):
            got = [_plan_keys(monkeypatch, {"CVLM_GEMM_VARIANT": variant}, M, N, K, form, ws=ws if use_ws else None, w_il=True, a_il=a, out_il=a)
                   for a in (False, True)]
            assert got == [_twin_of(want, "w"), _twin_of(want, "wa")], (M, N, K, form, got)


RING_PARAMS = ((581, 1024, 1024, "0"), (581, 1024, 4096, "4"), (300, 264, 96, "0"), (581, 3072, 1024, "0"), (130, 1024, 64, "0"),
               (581, 1024, 1024, "1"))
RING_SETTINGS = (("2", "0"), ("3", "0"), ("4", "0"), ("5", "0"), ("4", "1"), ("4", "2"), ("4", "3"))       # (CVLM_GEMM_RING, CVLM_GEMM_W8)
RING_KERNELS = (("r2",), ("r3",), ("r4",), ("r5",), ("w64",), ("w64",), ("w128",))
RING_KERNELS_SK4 = (("sk_r2/sk4",), ("sk_r3/sk4",), ("sk_r4/sk4",), ("sk_r4/sk4",), ("sk_w8/sk4",), ("sk_w8/sk4",), ("sk_w8/sk4",))


def test_relation_small_grid_ring_depth(monkeypatch, ws):
    """test_gemm_small_grid_ring_depth (VARIANT=0, a workspace; every setting is compared with the first):

        (RING, W8)       (2, 0)   (3, 0)   (4, 0)   (5, 0)   (4, 1)   (4, 2)   (4, 3)
        SK = 0 or 1      r2       r3       r4       r5       w64      w64      w128        all five parametrisations alike
        SK = 4           sk_r2    sk_r3    sk_r4    sk_r4    sk_w8    sk_w8    sk_w8       581 x 1024 x 4096, 4 parts

    Every setting after the first runs another instantiation than the two-slot loop.  With K-parts a ring of five is clamped to four
    slots, and W8 = 1 picks the 64-row form in all of them (never w128, which only W8 = 3 reaches here)."""
    assert _params("test_gemm_small_grid_ring_depth") == RING_PARAMS
    for M, N, K, sk in RING_PARAMS:
        got = tuple(_plan_keys(monkeypatch, {"CVLM_GEMM_SK": sk, "CVLM_GEMM_RING": r, "CVLM_GEMM_W8": w8}, M, N, K, "f32", ws=ws)
                    for r, w8 in RING_SETTINGS)
        assert got == (RING_KERNELS_SK4 if sk == "4" else RING_KERNELS), (M, N, K, sk, got)
        assert all(k != got[0] for k in got[1:])
