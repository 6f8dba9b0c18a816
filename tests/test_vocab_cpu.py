"""CPU: what class vocabularies at run time rest on that needs no GPU -- the pure request checks
(`vocabulary_request`, `decode_request(rank_cap=)`), the argument checks of the three C-ABI entries (they refuse before they touch a
device), and the vocabulary oracle (tests/vocab_oracle.py) against the reference's own run over 1100 classes
(tests/golden/tiny_vocab.npz, tools/make_vocab_golden.py)."""
import os

import numpy as np
import pytest
import torch

from camouflaged_vlm_amd import hip, spec, synth
from camouflaged_vlm_amd.engine import decode_request, vocabulary_request
from oracle import cvlm_oracle as O
import vocab_oracle as VO


def d(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max())


# ---- request checks ------------------------------------------------------------------------------------------------------------
CL, W, NCTX, D, V = 77, 8, 4, 6, 11


def _tokens(n=3):
    t = np.zeros((n, CL), np.int64)
    for i in range(n):
        t[i, :6 + i] = 1 + np.arange(6 + i) % 9
        t[i, 6 + i] = V - 1                                       # the EOT id is the largest: argmax finds its column
    return t


def test_vocabulary_request_accepts():
    base = dict(context_length=CL, text_width=W, n_ctx=NCTX, embed_dim=D)
    tok, table = _tokens(), torch.zeros(V, W)
    n, eot, ids = vocabulary_request(**base, tokens=tok, table=table)
    assert n == 3 and eot == [6, 7, 8] and ids.dtype == np.int32 and ids.flags["C_CONTIGUOUS"] and np.array_equal(ids, tok)
    n, eot, ids = vocabulary_request(**base, tokens=torch.from_numpy(tok).int(), table=table, eot=[9, 9, 76], bank=torch.zeros(3, D))
    assert eot == [9, 9, 76] and np.array_equal(ids, tok)
    n, eot, ids = vocabulary_request(**base, embeddings=torch.zeros(2, CL, W), eot=np.array([5, 20], np.int32), chunk=1)
    assert (n, eot, ids) == (2, [5, 20], None)
    assert vocabulary_request(**base, embeddings=torch.zeros(1, CL, W), eot=torch.tensor([NCTX + 1]))[1] == [NCTX + 1]


def test_vocabulary_request_rejects():
    base = dict(context_length=CL, text_width=W, n_ctx=NCTX, embed_dim=D)
    tok, table, emb = _tokens(), torch.zeros(V, W), torch.zeros(3, CL, W)
    over, neg = tok.copy(), tok.copy()
    over[1, 2], neg[0, 0] = V, -1
    bad = [dict(), dict(tokens=tok, table=table, embeddings=emb, eot=[6, 7, 8]),              # none or both of the forms
           # tokens: host ints of shape (n, context_length), ids in [0, V)
           dict(tokens=tok.astype(np.float32), table=table), dict(tokens=tok[:, :20], table=table), dict(tokens=tok[0], table=table),
           dict(tokens=tok != 0, table=table), dict(tokens=over, table=table), dict(tokens=neg, table=table),
           dict(tokens=tok[:0], table=table),
           # table: f32 (V, text_width), and only with tokens
           dict(tokens=tok), dict(tokens=tok, table=table.double()), dict(tokens=tok, table=torch.zeros(V, W + 1)),
           dict(tokens=tok, table=torch.zeros(V)), dict(tokens=tok, table=table.numpy()), dict(embeddings=emb, eot=[6, 7, 8], table=table),
           # embeddings: f32 (n, context_length, text_width), eot required
           dict(embeddings=emb), dict(embeddings=emb.double(), eot=[6, 7, 8]), dict(embeddings=emb[:, :9], eot=[6, 7, 8]),
           dict(embeddings=torch.zeros(3, CL, W + 1), eot=[6, 7, 8]), dict(embeddings=emb.numpy(), eot=[6, 7, 8]),
           dict(embeddings=emb[:0], eot=[]),
           # eot: n ints with n_ctx < eot < context_length
           dict(embeddings=emb, eot=[6, 7]), dict(embeddings=emb, eot=[6.0, 7.0, 8.0]), dict(embeddings=emb, eot=[6, NCTX, 8]),
           dict(embeddings=emb, eot=[6, CL, 8]), dict(embeddings=emb, eot=[-1, 7, 8]), dict(tokens=tok, table=table, eot=[3, 7, 8]),
           dict(tokens=np.zeros((2, CL), np.int64), table=table),                              # argmax of an all-zero row is column 0
           # bank: f32 (n, D) or None
           dict(embeddings=emb, eot=[6, 7, 8], bank=torch.zeros(2, D)), dict(embeddings=emb, eot=[6, 7, 8], bank=torch.zeros(3, D + 1)),
           dict(embeddings=emb, eot=[6, 7, 8], bank=torch.zeros(3, D, dtype=torch.float64)), dict(embeddings=emb, eot=[6, 7, 8], bank=np.zeros((3, D), np.float32)),
           # chunk
           dict(embeddings=emb, eot=[6, 7, 8], chunk=0), dict(embeddings=emb, eot=[6, 7, 8], chunk=2.0), dict(embeddings=emb, eot=[6, 7, 8], chunk=True)]
    for kw in bad:
        with pytest.raises(ValueError):
            vocabulary_request(**base, **kw)


def test_decode_request_rank_cap():
    base = dict(same_engine=True, B=2, D=8)
    with pytest.raises(ValueError):                               # today's default stays: 1024 classes are ranked
        decode_request(**base, n_cls=1025, topk=1)
    assert decode_request(**base, n_cls=1024, topk=1024) == ([0, 1], 1024, None)
    assert decode_request(**base, n_cls=1025, topk=1, rank_cap=65536) == ([0, 1], 1, None)
    assert decode_request(**base, n_cls=65536, topk=64, rank_cap=65536) == ([0, 1], 64, None)
    assert decode_request(**base, n_cls=1024, topk=100, rank_cap=65536) == ([0, 1], 100, None)
    for kw in (dict(n_cls=1025, topk=65, rank_cap=65536), dict(n_cls=65537, topk=1, rank_cap=65536), dict(n_cls=4817, topk=0, rank_cap=65536)):
        with pytest.raises(ValueError):
            decode_request(**base, **kw)
    # explicit classes of any K at any n
    cls = torch.tensor([[4816] * 70, [0] * 70], dtype=torch.int64)
    assert decode_request(**base, n_cls=4817, classes=cls)[1] == 70
    with pytest.raises(ValueError):
        decode_request(**base, n_cls=4817, classes=torch.tensor([[4817], [0]], dtype=torch.int64))


# ---- the three entries refuse bad arguments before they touch a device ----------------------------------------------------------
def test_new_entries_are_exported_and_the_abi_stays():
    lib = hip.load()
    for name in ("cvlm_text_assemble", "cvlm_clip_head_wide", "cvlm_clip_head_wide_workspace_bytes", "cvlm_topk_select_wide"):
        assert name in hip.EXPORTS and hasattr(lib, name)
    assert hip.ABI_VERSION == 12 and lib.cvlm_abi_version() == 12


def test_text_assemble_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(ids=p, table=p, V=11, emb=None, ctx=p, n_ctx=4, pos=p, n=3, cl=77, L=9, W=64, out=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_text_assemble(a["ids"], a["table"], a["V"], a["emb"], a["ctx"], a["n_ctx"], a["pos"],
                                      a["n"], a["cl"], a["L"], a["W"], a["out"], None)
    bad = [dict(ids=None), dict(emb=p), dict(table=None), dict(V=0), dict(V=-3), dict(ctx=None), dict(pos=None), dict(out=None),
           dict(n=0), dict(n=-1), dict(cl=0), dict(L=0), dict(L=78), dict(W=0), dict(W=66), dict(W=-4), dict(n_ctx=-1), dict(n_ctx=77),
           dict(ids=None, table=None, emb=p, n=0), dict(n=1 << 20, L=77, W=768)]                      # an output of 2^31 bytes or more
    for kw in bad:
        assert call(**kw) == -1, kw


def test_clip_head_wide_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    need = lib.cvlm_clip_head_wide_workspace_bytes(17, 2500)
    assert need > 0
    ok = dict(img=p, txt=p, P=17, Cc=2500, D=768, img_n=p, logits=p, pred=p, sel=p, ws=p, nbytes=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_clip_head_wide(a["img"], a["txt"], 100.0, a["P"], a["Cc"], a["D"],
                                       a["img_n"], a["logits"], a["pred"], a["sel"], a["ws"], a["nbytes"], None)
    bad = [dict(img=None), dict(txt=None), dict(img_n=None), dict(logits=None), dict(pred=None), dict(sel=None), dict(ws=None),
           dict(P=0), dict(P=-1), dict(P=65536), dict(Cc=0), dict(Cc=-5), dict(Cc=65537), dict(D=0), dict(D=770), dict(D=1028),
           dict(nbytes=need - 1), dict(nbytes=0), dict(ws=4100)]
    for kw in bad:
        assert call(**kw) == -1, kw
    for P, Cc in ((0, 5), (5, 0), (65536, 5), (5, 65537), (-1, -1)):
        assert lib.cvlm_clip_head_wide_workspace_bytes(P, Cc) == -1
    assert lib.cvlm_clip_head_wide_workspace_bytes(1, 1) > 0
    assert lib.cvlm_clip_head_wide_workspace_bytes(65535, 65536) > 0


def test_topk_select_wide_refuses_bad_arguments_without_gpu():
    lib = hip.load()
    p = 4096
    ok = dict(logits=p, B=2, Cc=2500, K=5, txt=p, D=8, idx_in=None, idx_out=p, sel=p)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cvlm_topk_select_wide(a["logits"], a["B"], a["Cc"], a["K"], a["txt"], a["D"],
                                         a["idx_in"], a["idx_out"], a["sel"], None)
    for kw in (dict(logits=None), dict(idx_in=p), dict(txt=None), dict(idx_out=None), dict(sel=None), dict(B=0), dict(B=-1), dict(Cc=0), dict(Cc=65537),
               dict(K=0), dict(K=65), dict(Cc=3, K=4), dict(D=0), dict(D=6)):
        assert call(**kw) == -1, kw


# ---- the oracle against the reference's own run ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    with np.load(os.path.join(golden_dir, "tiny_vocab.npz")) as z:
        return {k: z[k] for k in z.files}


def vocab_inputs(gold, c):
    """(tokens (N, 77) int32, table f32 (49408, W), bank f32 (N, D)) of tiny_vocab.npz's vocabulary."""
    N = int(gold["n_cls"])
    tokens = np.zeros((N, c.context_length), np.int32)
    tokens[:, :gold["tokens"].shape[1]] = gold["tokens"]
    table = torch.from_numpy(synth.make_tensor("openai.token_embedding.weight", (49408, c.text_width), "embed", 0))
    return tokens, table, torch.from_numpy(synth.make_text_bank(N, c.embed_dim, "test"))


def test_golden_conditions(gold):
    N = int(gold["n_cls"])
    assert N == 1100 and gold["pass1_logits"].shape == (2, N) and gold["class_logits"].shape == (2, 2, N)
    assert np.array_equal(gold["tokens"].argmax(-1), gold["eot"])
    for b in range(2):
        order = np.argsort(-gold["pass1_logits"][b], kind="stable")
        top9 = gold["pass1_logits"][b][order[:9]]
        assert np.array_equal(order[:8], gold["top8"][b]) and np.array_equal(order[:2], gold["classes"][b])
        assert float(np.min(top9[:-1] - top9[1:])) >= 1e-3
        for k in range(2):
            s = np.sort(gold["class_logits"][b, k])[::-1]
            assert s[0] - s[1] >= 1e-3 and int(gold["class_logits"][b, k].argmax()) == int(gold["pred"][b, k])


def test_oracle_reproduces_reference_vocabulary(gold):
    g, c = spec.TINY_SAM, spec.TINY_CLIP
    sd = O.to_torch_sd(synth.make_full_state_dict(g, c))
    inp, ci, cm = (torch.from_numpy(t) for t in synth.make_inputs(g, c, 2))
    tokens, table, bank = vocab_inputs(gold, c)
    emb = table[torch.from_numpy(tokens).long()]
    eot = gold["eot"].tolist()
    with torch.no_grad():
        rows = VO.rows(sd, c, emb, eot, bank)
        r = VO.infer_classes(inp, ci, cm, sd, g, c, emb, eot, bank, classes=torch.from_numpy(gold["classes"]))
    B, K = gold["classes"].shape
    pos = gold["pos"]
    figs = {"rows": (d(rows[gold["row_idx"]], gold["rows"]), gold["rows"]),
            "pass1_logits": (d(r["pass1_logits"], gold["pass1_logits"]), gold["pass1_logits"]),
            "low_masks": (d(r["low_masks"], gold["low_masks"]), gold["low_masks"]),
            "low_edges": (d(r["low_edges"], gold["low_edges"]), gold["low_edges"]),
            "masks_at_pos": (d(r["masks"].reshape(B, K, -1)[:, :, pos], gold["masks_at_pos"]), gold["masks_at_pos"]),
            "class_logits": (d(r["logits"], gold["class_logits"]), gold["class_logits"])}
    print("vocabulary oracle vs reference:", {k: f"{v:.2e}" for k, (v, _) in figs.items()})
    for k, (v, ref) in figs.items():                               # 1e-5 of each array's scale, as tests/test_classes_cpu.py
        assert v <= 1e-5 * max(1.0, float(np.abs(ref).max())), k
    assert np.array_equal(r["pred"].numpy(), gold["pred"])
    assert np.array_equal(torch.topk(r["pass1_logits"], 8, dim=1).indices.numpy(), gold["top8"])
