"""The GEMM planner (csrc/gemm_plan.h) against the launches of the launcher it replaced.

tests/golden/gemm_plans.json.gz is a recording of the one-function `cvlm_gemm` that preceded the planner: that function was compiled
with its kernel launches replaced by a recorder and called, without a GPU (256 CUs assumed, as it did there), over
  - every distinct argument struct that the forwards issue -- bench.py at the demo geometry with 1 and 8 images per step (the fused
    16-image CLIP pass of the pipelined loop included) on the engine, drop-in and eval-loop surfaces, the tiny geometry, hires1536 at
    B = 4, in precisions mx and exact -- and every (struct, CVLM_GEMM_* environment) pair that tests/test_ops_gpu.py and
    tests/test_gemm_mx_gpu.py issue (CVLM_GEMM_VARIANT = 2 and 7 and their SK / RING / W8 / PERSIST / TAIL / COLSPLIT / T192
    combinations among them).  They were taken from hip.gemm_args while the real host code ran with the kernels switched off: the
    struct of a launch is made by host code from shapes alone;
  - a grid of M in 2..36864, N in 32..5152 and K in 64..5152 that crosses each threshold of the choice (4096 rows, one round of
    256 / 512 tiles, a last round of at most 128 tiles, K / 32 >= 4 S, more 192-row than 256-row tiles) in every operand / epilogue /
    store form: planes, weight image, activation image and mx operands; plain, LayerNorm-fold and h2-residual epilogues; f32, h2,
    image and mx outputs; head-major, pixel-shuffle, batched, split-1 and implicit convolution launches where the shape admits them;
  - argument structs that the validation refuses, at least one per refusal;
each with and without a workspace, under the default knobs, under every non-default value of LIVE_SWITCHES (tests/test_cascade_gpu.py),
under CVLM_GEMM_RING=5 and CVLM_GEMM_W8=2 (without which two instantiations are never chosen: all 49 are in the table) and under
CVLM_GEMM_VARIANT = 1, 2, 7 and 1 with CVLM_GEMM_SK=4; the tests' pairs under the tests' own environments as well.
A row is the return code and, per launch, the kernel instantiation (demangled name of the function that was launched), grid, block, dynamic
LDS bytes and the GemmParams fields group_m / tail_rem / tail_split / total_blocks / sk_parts / N / nbx / nby, plus whether the launch's
K-parts pass through the workspace.  `cvlm_debug_gemm_plan` must reproduce every row exactly.

The probe variants (CVLM_GEMM_VARIANT values that exist in -DCVLM_PROBES builds only) are NOT in the table, which is checked against the
product library: they were compared by hand, the same recording made from probe builds of both launchers under every probe variant."""
import ctypes as C
import gzip
import json
import os

import pytest
import torch

from camouflaged_vlm_amd import hip


@pytest.fixture(scope="module")
def table(golden_dir):
    with gzip.open(os.path.join(golden_dir, "gemm_plans.json.gz"), "rt") as f:
        return json.load(f)


def _struct(rec: dict) -> hip.GemmArgs:
    """A recorded struct: pointer fields are 0 / 1 (NULL / given) -- the planner looks at nothing else of a pointer."""
    g = hip.GemmArgs()
    for i, (name, ctype) in enumerate(hip.GemmArgs._fields_):
        v = rec.get(name, 0)
        setattr(g, name, (0x1000000 * (i + 1) if v else None) if ctype is C.c_void_p else v)
    return g


def _plan(lib, g: hip.GemmArgs, have_ws: int, cus: int, fields):
    info = hip.GemmPlanInfo()
    rc = lib.cvlm_debug_gemm_plan(C.byref(g), have_ws, cus, C.byref(info))
    return [rc, [[l.kernel.decode() if f == "kernel" else getattr(l, f) for f in fields] for l in info.launch[:info.launches]]]


def test_every_recorded_plan_is_reproduced(table, monkeypatch):
    assert os.environ.get("CVLM_GEMM_VARIANT_LIVE") == "1", "tests/conftest.py: the knobs are re-read per call"
    lib = hip.load()
    fields, kernels = table["launch_fields"], table["kernels"]
    assert [n for n, _ in hip.GemmArgs._fields_] == table["arg_fields"]
    want = [[rc, [[kernels[l[0]]] + l[1:] for l in launches]] for rc, launches in table["plans"]]
    structs = [_struct(r) for r in table["args"]]
    checked, wrong = 0, []
    for env_i, have_ws, rows in table["cases"]:
        for name in [n for n in os.environ if n.startswith("CVLM_GEMM_") and n != "CVLM_GEMM_VARIANT_LIVE"]:
            monkeypatch.delenv(name)
        for name, value in table["envs"][env_i].items():
            monkeypatch.setenv(name, value)
        # a row list is one plan index per struct, in order (the sweep), or [struct, plan] pairs (the tests' own environments)
        for arg_i, plan_i in (rows if rows and isinstance(rows[0], list) else enumerate(rows)):
            got = _plan(lib, structs[arg_i], have_ws, table["cus"], fields)
            checked += 1
            if got != want[plan_i] and len(wrong) < 10:
                wrong.append((table["envs"][env_i], have_ws, table["args"][arg_i], "recorded", want[plan_i], "planned", got))
    assert not wrong, wrong
    assert checked == sum(len(rows) for _, _, rows in table["cases"]) and checked > 100000
    assert {rc for rc, _ in want} == {0, -1, -2}                       # launched, CVLM_E_BADARG, CVLM_E_UNSUPPORTED


def test_lds_bytes_of_a_plan_are_what_the_launch_passes(table):
    """By construction: the plan's lds_bytes and the launch helper's dynamic-LDS argument are the same constexpr function
    (gemm_lds_bytes, csrc/gemm_plan.h) of the kernel's template arguments, and the recorded rows above compare it with what the former
    launcher passed to every launch.  Here: one size per instantiation, and a handful against the sizes the former launcher spelled out."""
    fields, kernels = table["launch_fields"], table["kernels"]
    k_i, lds_i = fields.index("kernel"), fields.index("lds_bytes")
    per_kernel = {}
    for _, launches in table["plans"]:
        for l in launches:
            per_kernel.setdefault(kernels[l[k_i]], set()).add(l[lds_i])
    assert all(len(v) == 1 for v in per_kernel.values()), per_kernel
    known = {
        "gemm_nt_kernel<3, 2, 2, 2, 32, 0, 4, false, -1, false, false, false, false, false>": 2 * 2 * (128 + 128) * 32 * 2,
        "gemm_nt_kernel<1, 4, 2, 3, 32, 0, 4, false, -1, false, false, false, false, false>": 3 * 1 * (256 + 128) * 32 * 2,
        "gemm_nt_kernel<3, 4, 1, 2, 32, 0, 4, false, -1, true, false, false, false, false>": 2 * 2 * (256 + 64) * 32 * 2,
        "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 8, false, 1, false, false, true, false, false>": 2 * 2 * (256 + 256) * 32 * 2,
        "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 8, true, 1, false, false, true, false, false>": 2 * 2 * (256 + 256) * 32 * 2 + 8 * 16 * 64 * 4,
        "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 6, false, 2, false, false, true, false, false>": 2 * 2 * (192 + 256) * 32 * 2,
        "gemm_nt_kernel<3, 4, 2, 14, 32, 0, 2, false, -1, false, true, true, false, false>": 4 * 2 * (128 + 128) * 32 * 2,
        "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 8, false, 1, false, false, true, true, true>": 5 * 32768,
    }
    for name, lds in known.items():
        assert per_kernel[name] == {lds}, (name, per_kernel[name], lds)


def test_hip_gemm_plan_takes_the_arguments_of_hip_gemm(monkeypatch):
    """lin1 of a ViT-H block for one image (16 x 20 tiles of 256^2 on 256 CUs): one round of 256^2 tiles + the remaining columns as 128^2
    tiles; host tensors -- nothing is launched, nothing dereferenced."""
    for name in [n for n in os.environ if n.startswith("CVLM_GEMM_") and n != "CVLM_GEMM_VARIANT_LIVE"]:
        monkeypatch.delenv(name)
    M, N, K = 4096, 5120, 1280
    a, w, out = hip.H2.empty(M, K, device="cpu"), hip.H2.empty(N, K, device="cpu"), hip.H2.empty(M, N, device="cpu")
    stats, colsum = torch.empty(M, 2), torch.empty(N)
    plan = hip.gemm_plan(a, w, M, N, K, out_h2=out, ln_fold=(stats, colsum), act=hip.ACT_GELU, w_il=hip.interleave_planes(w))
    assert [(p["n0"], p["N"], p["grid_x"], p["block"]) for p in plan] == [(0, 4096, 256, 512), (4096, 1024, 256, 512)]
    assert plan[0]["kernel"] == "gemm_nt_kernel<3, 2, 4, 5, 32, 0, 8, false, 1, false, false, true, false, false>"
    assert plan[1]["kernel"] == "gemm_nt_kernel<3, 4, 2, 14, 32, 0, 2, false, -1, false, false, true, false, false>"
    with pytest.raises(RuntimeError):
        hip.gemm_plan(a, w, M, N, K + 8, out_h2=out)
