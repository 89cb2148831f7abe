"""What the model classes over HipBertEncoder share (bienc, sentenc, sbert, baselines, consent, contextner, polyenc, models): loading
the HF model and tokenizer, the checked read-out, the bucketed sentence encode, the per-paper split, filling a RepStore, the sentence
facet filter, otAspire as a similarity, checkpoint keys, run_info.json, and the frame of encode_to_pool.  Host-side Python only.

A model class writes its own tokenisation, its read-out (which HipBertEncoder.forward_* it calls and what of the result it judges and
returns) and its similarity; the rest it takes from here.
"""
import codecs
import json
import os

import numpy as np
import torch

from .batch_prep import pad_sentences, sentence_buckets


# ---- loading ------------------------------------------------------------------------------------------------------------------
def load_hf(name, model=None, tokenizer=None, want_tokenizer=True):
    """(model, tokenizer): AutoModel.from_pretrained(name) unless `model` is handed in; AutoTokenizer.from_pretrained(name) when a
    tokenizer is wanted, none is handed in and a name is known.  transformers is imported only when something is loaded."""
    if model is None:
        from transformers import AutoModel
        model = AutoModel.from_pretrained(name)
    if want_tokenizer and tokenizer is None and name is not None:
        from transformers import AutoTokenizer
        tokenizer = AutoTokenizer.from_pretrained(name)
    return model, tokenizer


# ---- the checked read-out -----------------------------------------------------------------------------------------------------
def all_finite(*tensors):
    """Every element of every tensor (None: skipped) is finite: one reduction per tensor, ONE host sync for the lot."""
    ok = None
    for t in tensors:
        if t is not None:
            f = torch.isfinite(t).all()
            ok = f if ok is None else ok & f
    return True if ok is None else bool(ok)


def _finite(result):
    return all_finite(*result) if isinstance(result, (tuple, list)) else all_finite(result)


class EncoderFront:
    """Base of the classes that own a `bert_encoder` (a HipBertEncoder); no other attribute is used."""

    def eval(self):
        return self

    def __call__(self, *args, **kwargs):
        return self.forward(*args, **kwargs)

    def _build_encoder(self, bert_model, matmul='fp32'):
        """self.bert_encoder over bert_model's weights.  matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16'
        (HipBertEncoder); every model class takes it as a keyword and hands it on here."""
        from .encoder import HipBertEncoder
        self.bert_encoder = HipBertEncoder(bert_model, matmul=matmul)

    def _rebuild_encoder(self, sd):
        """self.bert_encoder again from a BertModel state dict (a checkpoint), in the mode the model was built with."""
        from .encoder import HipBertEncoder
        self.bert_encoder = HipBertEncoder.from_state_dict(self.bert_encoder.config, sd, matmul=self.bert_encoder.matmul_asked)

    def _checked_read(self, read, finite_part, tok, typ, msk, who=None):
        """int64 [B, L] inputs (any device) to the GPU once, then read(tok, typ, msk) under the encoder's fall-back rule
        (encoder.run_checked), which judges finite_part(result): a tensor or a tuple of tensors (None entries skipped)."""
        enc = self.bert_encoder
        tok, typ, msk = enc.device_inputs(tok, typ, msk)
        return enc.checked(lambda: read(tok, typ, msk), lambda r: _finite(finite_part(r)), who or type(self).__name__)

    def _checked_fill(self, fill, total, who):
        """encode_to_pool's store, fill() -> rows or (rows, CLS reps or None), under the fall-back rule once: one status read and one
        finite check for the whole corpus.  An empty store (total 0) is just made."""
        return self.bert_encoder.checked(fill, _finite, who) if total else fill()


# ---- sentences ----------------------------------------------------------------------------------------------------------------
def encode_bucketed(read_run, ids, types, pad_id, max_tokens, device):
    """Sentences given as id / token type lists -> float32 [N, 768] on `device`, in input order.  The sentences are sorted by token
    count and cut into encoder calls of at most max_tokens padded token rows (batch_prep.sentence_buckets), each padded with pad_id
    to its own longest member; read_run(tok, typ, msk) gives a call's [n, 768] reps on `device`."""
    out = torch.empty(len(ids), 768, device=device, dtype=torch.float32)
    for run in sentence_buckets([len(x) for x in ids], max_tokens):
        out[torch.from_numpy(run).to(device)] = read_run(*pad_sentences(ids, types, run, pad_id))
    return out


def per_paper(batch_papers, encode_sentences):
    """The ABSTRACT sentences of all papers in one list, encode_sentences(list) -> np [N, 768], split back per paper with np.split
    semantics: a list of float32 [n_sents, 768] (a paper without sentences: [0, 768]; no sentence at all: no encode call)."""
    batch, splits = [], []
    for paper in batch_papers:
        batch += list(paper['ABSTRACT'])
        splits.append(len(batch))
    reps = encode_sentences(batch) if batch else np.zeros((0, 768), np.float32)
    return np.split(reps, splits[:-1])


def facet_sentence_ids(facet_labels, facet):
    """The numbers of the sentences labelled `<facet>_label`; 'objective_label' counts as background (models.py:147-153)."""
    labels = ['background' if lab == 'objective_label' else lab[:-len('_label')] for lab in facet_labels]
    return [i for i, k in enumerate(labels) if facet == k]


def sentence_facet_rows(unfaceted_encoding, facet, input_data):
    """SimilarityModel.get_faceted_encoding for encoding_type 'sentence' (models.py:147-153): the facet's sentence rows."""
    return unfaceted_encoding[facet_sentence_ids(input_data['FACETS'], facet)]


def ot_similarity(x, y):
    """AspireModel.get_similarity (models.py:190-197): the negative Wasserstein distance of two [n, 768] rep matrices."""
    from .scorer import get_similarity
    return get_similarity(x, y)


# ---- rep stores ---------------------------------------------------------------------------------------------------------------
def check_pid_count(pids, n, what='papers'):
    if len(pids) != n:
        raise ValueError(f'{len(pids)} pids for {n} {what}')


def add_to_store(store, pids, blocks, what='papers'):
    """blocks[j] -- a row block [n, 768], or (rows, layout) as RepStore.add takes them -- added under pids[j] to `store` (None: a new
    RepStore).  blocks may be a generator that encodes as it goes; the counts are compared when it ends.  Returns the store."""
    from .repstore import RepStore
    store = RepStore() if store is None else store
    pids = list(pids)
    n = 0
    for block in blocks:
        store.add(pids[n], *(block if isinstance(block, tuple) else (block,)))
        n += 1
    check_pid_count(pids, n, what)
    return store


# ---- checkpoints --------------------------------------------------------------------------------------------------------------
def refuse_keys(keys, who):
    if keys:
        raise KeyError(f'unexpected keys in the {who} state dict: {keys}')


def strip_prefix(sd, prefix, drop=(), who=None):
    """A checkpoint's state dict -> ({key without `prefix`: value}, [the keys that start neither with it nor with one of `drop`]).
    who: any such key is a KeyError naming it."""
    stripped = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
    other = [k for k in sd if not k.startswith((prefix,) + tuple(drop))]
    if who is not None:
        refuse_keys(other, who)
    return stripped, other


def read_hparams(run_dir):
    """A training run's hyper-parameters: run_info.json's 'all_hparams'."""
    with codecs.open(os.path.join(run_dir, 'run_info.json'), 'r', 'utf-8') as fp:
        return json.load(fp)['all_hparams']


# ---- the frame of encode_to_pool ------------------------------------------------------------------------------------------------
def pool_layout(all_lens):
    """Rows per document, corpus order -> (lens_t, start_t) int32 on the host: the store's CSR, and the row total."""
    lens_t = torch.tensor(all_lens, dtype=torch.int32)
    start_t = (torch.cumsum(lens_t, 0) - lens_t).to(torch.int32)
    return lens_t, start_t, int(sum(all_lens))


def check_token_ids(batches_of_tokid, vocab_size, device):
    """The token ids of every batch validated with ONE device round trip (nn.Embedding raises IndexError on the reference path); per
    batch that check is a host sync in front of every encoder call.  64 batches' ids are flattened into one tensor per reduction:
    per batch it was two tiny kernels each, ~1000 launches in front of the first encoder call of a 16 384-document corpus."""
    toks = list(batches_of_tokid)
    if toks:
        lo_hi = torch.stack([torch.stack(torch.aminmax(torch.cat([t.reshape(-1) for t in toks[i:i + 64]]))).to(device)
                             for i in range(0, len(toks), 64)])
        if int(lo_hi[:, 0].min()) < 0 or int(lo_hi[:, 1].max()) >= vocab_size:
            raise IndexError('token id out of range')


def finish_pool(rows, lens_t, start_t, all_lens, pids, planes):
    """The filled row matrix with its CSR as a scorer.CandidatePool; planes: CandidatePool.prepare_planes on a store that has rows."""
    from . import ops
    from .scorer import CandidatePool
    dev = rows.device
    repset = ops.DeviceRepSet(rows, start_t.to(dev), lens_t.to(dev), ext=0, max_len=max(all_lens) if all_lens else 0,
                              lens_host=all_lens)
    pool = CandidatePool.from_repset(repset, pids=pids)
    if planes and rows.shape[0]:
        pool.prepare_planes()
    return pool
