"""CPU oracle of a class vocabulary made at run time (ClipModel.make_vocabulary, Cascade.*(vocab=)), composed from
oracle/cvlm_oracle.py's own functions.

A vocabulary replaces the prompt learner's test rows: token_prefix_test / token_suffix_test are the embedded prompts
`table[tokens]` cut around the learned context (cocotrainers/mapleAlphaCLIP.py:132-168: prefix = embedding[:, :1], suffix =
embedding[:, 1 + n_ctx:]), everything else of the model stays.  The text rows, pass 1, the K hypotheses and stage 2 then follow from
`O.clip_text_features` and tests/classes_oracle.py with that state dict and the vocabulary's bank."""
from __future__ import annotations

import torch

from oracle import cvlm_oracle as O
import classes_oracle as CO


def vocabulary_sd(sd, c, embeddings, prefix: str = "clip_model."):
    """Copy of `sd` whose test prompts are `embeddings` f32 (n, context_length, text_width) = table[tokens]."""
    out = dict(sd)
    pl = prefix + "prompt_learner."
    emb = torch.as_tensor(embeddings, dtype=torch.float32)
    out[pl + "token_prefix_test"] = emb[:, :1].clone()
    out[pl + "token_suffix_test"] = emb[:, 1 + c.n_ctx:].clone()
    return out


def text_features(sd, c, embeddings, eot):
    """(n, D) text tower output of the vocabulary's prompts (mapleAlphaCLIP.py:210-227, 64-78)."""
    return O.clip_text_features(vocabulary_sd(sd, c, embeddings), c, [int(e) for e in eot], truncate=True)


def rows(sd, c, embeddings, eot, bank):
    """(n, D) normalise(text features) + bank (:289-291)."""
    return CO.text_rows(text_features(sd, c, embeddings, eot), torch.as_tensor(bank))


def infer_classes(inp, clip_image, clip_mask, sd, g, c, embeddings, eot, bank, classes=None, topk=None):
    """tests/classes_oracle.infer_classes against the vocabulary: same dict of outputs, n = the vocabulary's size."""
    tf = text_features(sd, c, embeddings, eot)
    return CO.infer_classes(inp, clip_image, clip_mask, vocabulary_sd(sd, c, embeddings), g, c, tf, torch.as_tensor(bank),
                            classes=classes, topk=topk)
