"""The split-1 GEMM cases (tests/gemm_split1_cases.py) planned without a GPU: every case reaches the instantiation it names, the table
covers every split-1 instantiation the library has, and which of them the launches of the real forwards reach."""
import os
import re

import gemm_split1_cases as S1
from camouflaged_vlm_amd import hip

PLAN_H = os.path.join(os.path.dirname(os.path.abspath(hip.__file__)), "csrc", "gemm_plan.h")


def _clean_env(monkeypatch, variant):
    for name in [n for n in os.environ if n.startswith("CVLM_GEMM_") and n != "CVLM_GEMM_VARIANT_LIVE"]:
        monkeypatch.delenv(name)
    if variant is not None:
        monkeypatch.setenv("CVLM_GEMM_VARIANT", variant)


def test_table_has_every_form_on_every_kernel():
    assert len({c.id for c in S1.CASES}) == len(S1.CASES)
    for k in S1.PLAIN_KERNELS:
        assert {c.form for c in S1.CASES if c.kernel == k} == {"product", "plain", "batched", "pixel_shuffle", "head_major", "ln_fold",
                                                                 "h2_residual"}
        for shape in S1.SHAPES:
            plain = [c for c in S1.of("plain", k) if c.shape == shape]
            assert {c.act for c in plain if c.layout == "tight"} == {0, 1, 2, 3}
            assert {c.layout for c in plain} == set(S1.LAYOUTS)
        assert {(c.shape, c.nolo) for c in S1.of("head_major", k)} == {(s, n) for s in S1.HEAD_MAJOR_SHAPES for n in (0, 2, 5)}
        assert {(c.shape, c.act) for c in S1.of("ln_fold", k)} == {(s, a) for s in S1.STAGED_SHAPES for a in (0, 1, 2)}
        assert {c.shape for c in S1.of("h2_residual", k)} == set(S1.STAGED_SHAPES)
    assert len(S1.STAGED_SHAPES) == 3 and all(s[1] % 64 == 8 for s in S1.STAGED_SHAPES)      # N = 264, 392: the last piece has 8 columns


def test_every_case_reaches_the_kernel_it_names(monkeypatch):
    """Under the case's CVLM_GEMM_VARIANT the planner gives one launch of the named instantiation -- for the very arguments the GPU test
    passes to hip.gemm.  Over the table: exactly the split-1 entries of CVLM_GEMM_KERNELS (csrc/gemm_plan.h), so a fifth split-1
    instantiation without a case fails here."""
    assert os.environ.get("CVLM_GEMM_VARIANT_LIVE") == "1", "tests/conftest.py: the knobs are re-read per call"
    reached = set()
    for c in S1.CASES:
        _clean_env(monkeypatch, None if c.kernel == "conv" else c.kernel)
        L = S1.launch(c, hip, "cpu")
        plan = hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, **L.kw)
        assert len(plan) == 1 and plan[0]["kernel"] == S1.KERNELS[c.kernel], (c.id, plan)
        assert plan[0]["sk_parts"] == 1 and plan[0]["tail_rem"] == 0 and not plan[0]["uses_workspace"], (c.id, plan)
        reached.add(plan[0]["kernel"])
        if c.form == "head_major":                                  # the plain h2 launch it is compared with: the same kernel
            kw = {k: v for k, v in L.kw.items() if k not in ("head_major", "head_major_nolo")}
            assert hip.gemm_plan(L.A, L.W, L.M, L.N, L.K, **kw)[0]["kernel"] == S1.KERNELS[c.kernel]
    with open(PLAN_H) as f:
        text = f.read()
    body = text[text.index("#define CVLM_GEMM_KERNELS(X)"):text.index("#define CVLM_X_IL(")]
    split1 = [m for m in re.findall(r"\bX\(([^()]*)\)", body) if m.split(",")[0].strip() == "1"]
    dflt = ["", "", "", "", "", "0", "4", "false", "-1", "false", "false", "false", "false", "false"]
    names = set()
    for m in split1:
        args = [a.strip() for a in m.split(",")]
        names.add("gemm_nt_kernel<" + ", ".join(args + dflt[len(args):]) + ">")
    assert len(split1) == 4 and names == set(S1.KERNELS.values()) == reached


# The split-1 GEMM launches of the real forwards (demo geometry: ViT-H at 1024 px, CLIP ViT-L/14 at 336 px with 4 context tokens, 61
# test classes, decoder at 64 x 64): (name, M per image or fixed M, N, K, per_image)
REAL_SHAPES = (
    ("ViT-H qkv", 4096, 3840, 1280, True),
    ("ViT-H proj", 4096, 1280, 1280, True),
    ("ViT-H lin1", 4096, 5120, 1280, True),
    ("ViT-H lin2", 4096, 1280, 5120, True),
    ("CLIP vision in_proj", 581, 3072, 1024, True),
    ("CLIP vision out_proj", 581, 1024, 1024, True),
    ("CLIP vision c_fc", 581, 4096, 1024, True),
    ("CLIP vision c_proj", 581, 1024, 4096, True),
    ("CLIP text in_proj", 77 * 61, 2304, 768, False),
    ("CLIP text out_proj", 77 * 61, 768, 768, False),
    ("CLIP text c_fc", 77 * 61, 3072, 768, False),
    ("CLIP text c_proj", 77 * 61, 768, 3072, False),
    ("decoder up-scaling 1", 4096, 256, 256, True),
    ("decoder up-scaling 2", 16384, 128, 64, True),
    ("hypernetwork layers 0/1", 1, 256, 256, True),
    ("hypernetwork tail", 1, 32, 256, True),
)
# which of the three plain kernels (the CVLM_GEMM_VARIANT that names it) the planner picks for them on 256 CUs, batch 1 and batch 8
REAL_PICKS = {
    "ViT-H qkv": ("5", "5"),
    "ViT-H proj": ("2", "2"),
    "ViT-H lin1": ("2", "5"),
    "ViT-H lin2": ("2", "2"),
    "CLIP vision in_proj": ("2", "5"),
    "CLIP vision out_proj": ("2", "2"),
    "CLIP vision c_fc": ("2", "2"),
    "CLIP vision c_proj": ("2", "2"),
    "CLIP text in_proj": ("2", "2"),
    "CLIP text out_proj": ("2", "2"),
    "CLIP text c_fc": ("5", "5"),
    "CLIP text c_proj": ("2", "2"),
    "decoder up-scaling 1": ("2", "2"),
    "decoder up-scaling 2": ("2", "2"),
    "hypernetwork layers 0/1": ("2", "2"),
    "hypernetwork tail": ("2", "2"),
}


def _real_picks(monkeypatch):
    _clean_env(monkeypatch, "0")
    by_name = {v: k for k, v in S1.KERNELS.items()}
    got = {}
    for name, m, N, K, per_image in REAL_SHAPES:
        picks = []
        for B in (1, 8):
            M = m * B if per_image else m
            a = w = out = hip.H2.empty(1, 8, device="cpu")          # nothing is dereferenced: the planner reads shapes and NULL / given
            plan = hip.gemm_plan(a, w, M, N, K, out_h2=out, split=1)
            assert len(plan) == 1
            picks.append(by_name[plan[0]["kernel"]])
        got[name] = tuple(picks)
    return got


def test_which_kernels_real_launches_reach(monkeypatch):
    """Under CVLM_GEMM_VARIANT=0 on 256 CUs (for split 1 the choice is a function of M, N and the batch alone: big_grid_variant,
    csrc/gemm_plan.h).  B = images per forward; the text tower runs the 61 test classes whatever B is.

        launch                     M x N x K                  B = 1      B = 8
        ViT-H qkv                  4096 B x 3840 x 1280       256^2      256^2
        ViT-H proj                 4096 B x 1280 x 1280       256x128    256x128
        ViT-H lin1                 4096 B x 5120 x 1280       256x128    256^2
        ViT-H lin2                 4096 B x 1280 x 5120       256x128    256x128
        CLIP vision in_proj        581 B x 3072 x 1024        256x128    256^2
        CLIP vision out_proj       581 B x 1024 x 1024        256x128    256x128
        CLIP vision c_fc           581 B x 4096 x 1024        256x128    256x128
        CLIP vision c_proj         581 B x 1024 x 4096        256x128    256x128
        CLIP text in_proj          4697 x 2304 x 768          256x128    256x128
        CLIP text out_proj         4697 x 768 x 768           256x128    256x128
        CLIP text c_fc             4697 x 3072 x 768          256^2      256^2
        CLIP text c_proj           4697 x 768 x 3072          256x128    256x128
        decoder up-scaling 1       4096 B x 256 x 256         256x128    256x128
        decoder up-scaling 2       16384 B x 128 x 64         256x128    256x128
        hypernetwork layers 0 / 1  B x 256 x 256              256x128    256x128
        hypernetwork tail          B x 32 x 256               256x128    256x128

    The 256 x 128 kernel (variant 2) and the 256^2 kernel (variant 5) are reached.  The 128^2 kernel (variant 1, gemm_nt_kernel<1, 2, 2,
    2, 32>) is reached by NONE of these launches: under one round of tiles the model's c2 = 256 * 2 / 1.05 = 487 always beats c1 = 512.
    It runs only when CVLM_GEMM_VARIANT=1 forces it."""
    got = _real_picks(monkeypatch)
    assert got == REAL_PICKS, got
