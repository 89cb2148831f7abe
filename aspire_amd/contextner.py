"""The entity-augmented Aspire models of the reference's evaluation factory (src/evaluation/utils/models.py:738-768, encoding type
'sentence-entity'):

  * ``AspireContextNER`` + ``AspireConSenContextual`` (aspire_context_ner_*; models.py:413-508, 607-735): ONE BERT forward per
    abstract, then besides every sentence span one row per named entity -- the mean of the last-layer token rows inside the
    entity's span.  A paper is ``[sentence rows ; valid entity rows]``, scored by otAspire.
  * ``AspireNER`` (aspire_ner_*; models.py:211-233): the entity strings appended to the abstract as further sentences, encoded by
    AspireConSent.

    model = AspireContextNER('allenai/aspire-contextualsentence-multim-compsci')
    reps = model.encode(batch_papers)                       # per paper [n_sents + n_valid_entities, 768]
    sim = model.get_similarity(reps[0], reps[1])
    query = model.get_faceted_encoding(reps[0], 'method', batch_papers[0])

Papers are dicts with 'TITLE', 'ABSTRACT' (sentences), 'ENTITIES' (per sentence a list of entity strings) and, for the facet
filter, 'FACETS' (per sentence a label).  The forward runs in HipBertEncoder, all the pooling of a call in ONE launch of
aspire_span_pool_ranges_f32 (include/aspire_hip.h): sentence and entity spans are ranges of token rows, the kernel's grid is
over the rows that exist.  ``encode_to_pool`` / ``encode_to_store`` are the device-resident route: the rows of every paper are
written consecutively into the candidate pool's row matrix in HBM.
"""
import numpy as np
import torch

from . import ops
from .batch_prep import append_entities, prepare_abstracts_entities, span_range_tables
from .consent import AspireConSent
from .model_front import (EncoderFront, add_to_store, all_finite, check_pid_count, check_token_ids, facet_sentence_ids, finish_pool,
                          load_hf, ot_similarity, pool_layout)


# ---- the 'sentence-entity' facet filter (host side, integers only) ---------------------------------------------------------
def facet_row_ids(facet_labels, entities, facet):
    """SimilarityModel.get_faceted_encoding for encoding type 'sentence-entity' (models.py:127-163) as row numbers: the sentences
    labelled `<facet>_label` (model_front.facet_sentence_ids), then the entity rows of those sentences, entity rows being
    counted from len(facet_labels) in sentence order.  entities: per sentence the list of its entities (only its length is used)."""
    sent_ids = facet_sentence_ids(facet_labels, facet)
    ner_cur_id = len(facet_labels)
    ner_ids = []
    for i, sent_ners in enumerate(entities):
        if i in sent_ids:
            ner_ids += list(range(ner_cur_id, ner_cur_id + len(sent_ners)))
        ner_cur_id += len(sent_ners)
    return sent_ids + ner_ids


def filter_valid_entities(entities, is_valid_entity):
    """The entity lists AspireContextNER.get_faceted_encoding hands to the base filter (models.py:719-728).  is_valid_entity: one
    flag per entity of the kept sentences (ner_token_idxs non-empty).  As in the reference the entity counter advances on VALID
    entities only: from the first invalid entity on, every later entity is compared with that same flag and dropped, and a paper
    whose flags run out (every kept entity valid, further entities in sentences the 500-piece cap dropped) raises IndexError."""
    filtered, entity_id = [], 0
    for sent_ners in entities:
        kept = []
        for entity in sent_ners:
            if is_valid_entity[entity_id]:
                kept.append(entity)
                entity_id += 1
        filtered.append(kept)
    return filtered


def _pooling_tables(sent_tok_idxs, ner_tok_idxs, max_seq_len, dev, row_base=None, pad_sents=None):
    """span_range_tables uploaded as ONE int32 buffer: ((doc, tok_start, tok_len, out_row or None) on the GPU, n_entities)."""
    (doc, start, length, out_row), n_entities = span_range_tables(sent_tok_idxs, ner_tok_idxs, row_base=row_base, pad_sents=pad_sents,
                                                                  max_seq_len=max_seq_len)
    parts = [doc, start, length] + ([out_row] if out_row is not None else [])
    flat = torch.from_numpy(np.stack(parts)).to(dev)
    return (flat[0], flat[1], flat[2], flat[3] if out_row is not None else None), n_entities


class AspireConSenContextual(EncoderFront):
    """Drop-in for the class of the same name (models.py:413-508): contextual sentence reps and contextual entity reps from one
    BERT forward."""

    def __init__(self, hf_model_name=None, bert_model=None, matmul='fp32'):
        """
        :param hf_model_name: HuggingFace model name or path, loaded like the reference does (models.py:422).
        :param bert_model: an already constructed transformers BertModel (weights are copied to the GPU).
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.bert_encoding_dim = 768
        self.bert_layer_count = 12 + 1  # plus 1 for the bottom most layer.
        self._build_encoder(load_hf(hf_model_name, bert_model, want_tokenizer=False)[0], matmul)

    def forward(self, bert_batch, abs_lens, sent_tok_idxs, ner_tok_idxs):
        """
        :return: sent_reps [batch_size x max_sents x 768], ner_reps: per paper a list with a [1, 768] tensor per entity that has
            token positions and [] per entity that has none (models.py:466-477)
        """
        _, sent_reps, ner_reps = self.consent_reps_bert(bert_batch=bert_batch, batch_senttok_idxs=sent_tok_idxs,
                                                        batch_nertok_idxs=ner_tok_idxs, num_sents=abs_lens)
        return sent_reps, ner_reps

    def consent_reps_bert(self, bert_batch, batch_senttok_idxs, batch_nertok_idxs, num_sents):
        """
        :param bert_batch: dict('tokid_tt', 'seg_tt', 'attnmask_tt', 'seq_lens')
        :param batch_senttok_idxs: list(list(list(int))); batch_size([num_sents_per_abs[num_tokens_in_sent]])
        :param batch_nertok_idxs: list(list(list(int))); batch_size([num_entities_per_abs[num_tokens_in_entity]]), [] = no positions
        :param num_sents: list(int); number of sentences in each example in the batch passed.
        :return: doc_cls_reps [batch_size x 768], sent_reps, ner_reps (forward)
        """
        seq_lens = bert_batch['seq_lens']
        batch_size, max_seq_len = len(seq_lens), max(seq_lens)
        max_sents = max(num_sents)
        tokid_tt, seg_tt, attnmask_tt = bert_batch['tokid_tt'], bert_batch['seg_tt'], bert_batch['attnmask_tt']
        out_dev = tokid_tt.device
        assert tokid_tt.shape == (batch_size, max_seq_len)
        enc = self.bert_encoder
        tok, typ, msk = enc.device_inputs(tokid_tt, seg_tt, attnmask_tt)
        # one buffer: the padded [B, S, 768] sentence block (slots beyond a paper's sentences are zero-length rows: exact zeros),
        # then the valid entities' rows in paper order
        (doc, start, length, _), n_entities = _pooling_tables(batch_senttok_idxs, batch_nertok_idxs, max_seq_len, enc.device,
                                                              pad_sents=max_sents)
        n_sent_rows = batch_size * max_sents
        out_row, ent0 = [], n_sent_rows
        for b, n_ent in enumerate(n_entities):
            out_row += list(range(b * max_sents, (b + 1) * max_sents)) + list(range(ent0, ent0 + n_ent))
            ent0 += n_ent
        out_row = torch.tensor(out_row, dtype=torch.int32).to(enc.device)

        def run():
            rows = torch.empty(ent0, 768, device=enc.device, dtype=torch.float32)
            cls = torch.empty(batch_size, 768, device=enc.device, dtype=torch.float32)
            ops.span_pool_ranges(enc.forward_hidden(tok, typ, msk, check_ids=False), doc, start, length, rows=rows, out_row=out_row,
                                 cls=cls)
            return cls, rows
        doc_cls_reps, rows = enc.checked(run, lambda r: all_finite(*r), 'AspireConSenContextual')
        sent_reps = rows[:n_sent_rows].view(batch_size, max_sents, 768).to(out_dev)
        ner_rows = rows[n_sent_rows:].to(out_dev)
        ner_reps, e = [], 0
        for paper in batch_nertok_idxs:
            paper_reps = []
            for ner_toks in paper:
                if len(ner_toks) > 0:
                    paper_reps.append(ner_rows[e:e + 1])
                    e += 1
                else:
                    paper_reps.append([])
            ner_reps.append(paper_reps)
        return doc_cls_reps.to(out_dev), sent_reps, ner_reps


class _SentenceEntityModel:
    """What the two 'sentence-entity' models share: otAspire as the similarity and the base facet filter."""
    encoding_type = 'sentence-entity'
    get_similarity = staticmethod(ot_similarity)

    def get_faceted_encoding(self, unfaceted_encoding, facet, input_data):
        """SimilarityModel.get_faceted_encoding (models.py:127-163): the rows of the facet's sentences and of their entities."""
        return unfaceted_encoding[facet_row_ids(input_data['FACETS'], input_data['ENTITIES'], facet)]


class AspireNER(_SentenceEntityModel):
    """aspire_ner_* (models.py:211-233): every entity string is one more sentence of the abstract; AspireConSent encodes the lot."""

    def __init__(self, hf_model_name=None, bert_model=None, tokenizer=None, name='aspire_ner_compsci', matmul='fp32'):
        self.name = name
        bert_model, self.tokenizer = load_hf(hf_model_name, bert_model, tokenizer)
        self.model = AspireConSent(bert_model=bert_model, matmul=matmul)

    def encode(self, batch_papers, tokenizer=None):
        """:return: per paper [n_kept_sentences (abstract sentences, then entity strings), 768]"""
        assert 'ENTITIES' in batch_papers[0], 'No NER data for input.'
        return self.model.encode(append_entities(batch_papers), tokenizer if tokenizer is not None else self.tokenizer)


class AspireContextNER(_SentenceEntityModel):
    """aspire_context_ner_* (models.py:607-735)."""

    def __init__(self, hf_model_name=None, bert_model=None, tokenizer=None, name='aspire_context_ner_compsci', matmul='fp32'):
        """
        :param hf_model_name: the HF model (and tokenizer) to load; the reference loads
            'allenai/aspire-contextualsentence-multim-compsci' (models.py:615).
        :param bert_model: an already constructed transformers BertModel instead (weights are copied to the GPU).
        :param tokenizer: default AutoTokenizer.from_pretrained(hf_model_name).
        :param matmul: the encoder's matmul mode, 'fp32' or the opt-in 'fp16' (HipBertEncoder).
        """
        self.name = name
        bert_model, self.tokenizer = load_hf(hf_model_name, bert_model, tokenizer)
        self.model = AspireConSenContextual(bert_model=bert_model, matmul=matmul)

    def _preprocess_input(self, input_data):
        return prepare_abstracts_entities(input_data, self.tokenizer)

    def prepare(self, batch_papers):
        """encode_to_pool's input for a batch of papers: _preprocess_input's four values plus, per paper, the entity count of every
        kept sentence (from which the pool's row layout is told)."""
        bert_batch, abs_lens, sent_idxs, ner_idxs = self._preprocess_input(batch_papers)
        ents = [[len(x) for x in list(p['ENTITIES'])[:n]] for p, n in zip(batch_papers, abs_lens)]
        return bert_batch, abs_lens, sent_idxs, ner_idxs, ents

    def encode(self, input_data):
        """models.py:620-639: papers -> per paper [n_sents + n_valid_entities, 768] (sentence rows, then the rows of the entities
        that have token positions, in order), on the CPU like the reference's."""
        bert_batch, abs_lens, sent_idxs, ner_idxs = self._preprocess_input(input_data)
        enc, tokid_tt = self.model.bert_encoder, bert_batch['tokid_tt']
        (doc, start, length, _), n_entities = _pooling_tables(sent_idxs, ner_idxs, tokid_tt.shape[1], enc.device)
        rows = self.model._checked_read(
            lambda tok, typ, msk: ops.span_pool_ranges(enc.forward_hidden(tok, typ, msk, check_ids=False), doc, start, length),
            lambda r: r, tokid_tt, bert_batch['seg_tt'], bert_batch['attnmask_tt'], 'AspireContextNER')
        rows = rows.to(tokid_tt.device)
        return list(torch.split(rows, [n + e for n, e in zip(abs_lens, n_entities)]))

    def get_faceted_encoding(self, unfaceted_encoding, facet, input_data):
        """models.py:708-734: the base filter on the paper with its entity lists cut to what filter_valid_entities keeps."""
        _, _, _, ner_idxs = self._preprocess_input([input_data])
        filtered = filter_valid_entities(input_data['ENTITIES'], [len(x) > 0 for x in ner_idxs[0]])
        return unfaceted_encoding[facet_row_ids(input_data['FACETS'], filtered, facet)]

    # ---- the device-resident route -------------------------------------------------------------------------------------
    def encode_to_pool(self, batches, pids=None, docs_per_forward=64, planes=False):
        """Encode paper batches straight into a resident candidate pool (the counterpart of AspireConSent.encode_to_pool).

        batches: iterable of ``prepare(batch_papers)`` tuples (or _preprocess_input's four values: then no per-sentence layout is
        returned).  The pool's row matrix [sum over papers of n_sents + n_valid_entities, 768] is allocated once in HBM; consecutive
        batches are joined into encoder calls of up to docs_per_forward papers (AspireConSent._merge_batches; None or 0: one call per
        batch as given) and after every encoder call ONE aspire_span_pool_ranges_f32 launch writes each paper's sentence rows and
        valid entity rows consecutively into the paper's rows of the store -- no padded tensor, no copy back to the host.  The
        pooling tables of all calls are built first and uploaded as one buffer.  The finished store goes through the encoder's
        fall-back rule (encoder.run_checked) once: one status read and one finite check; a re-run encodes everything again.
        planes: also keep the rows as fp16 planes (CandidatePool.prepare_planes).
        Returns (scorer.CandidatePool, layout): layout[j] = (n_sents, valid entity count per sentence, or None) of paper j.
        A paper of more than aspire_max_sents() rows is encoded; scoring it raises NotImplementedError."""
        dev = ops.require_gpu()
        batches = [tuple(b) for b in batches]
        layout, all_lens = [], []
        for item in batches:
            abs_lens, ner_idxs = item[1], item[3]
            ents = item[4] if len(item) > 4 else [None] * len(abs_lens)
            for n, paper_ners, paper_ents in zip(abs_lens, ner_idxs, ents):
                n_valid = sum(len(x) > 0 for x in paper_ners)
                per_sent = None
                if paper_ents is not None:
                    flags = iter(len(x) > 0 for x in paper_ners)
                    per_sent = [sum(next(flags) for _ in range(k)) for k in paper_ents]
                layout.append((int(n), per_sent))
                all_lens.append(int(n) + n_valid)
        lens_t, start_t, total = pool_layout(all_lens)
        enc = self.model.bert_encoder
        check_token_ids((item[0]['tokid_tt'] for item in batches), enc.config.vocab_size, dev)
        # (a paper's sentence and entity index lists travel through _merge_batches as one pair)
        triples = [(item[0], item[1], list(zip(item[2], item[3]))) for item in batches]
        forwards = AspireConSent._merge_batches(triples, docs_per_forward) if docs_per_forward else triples
        parts, spans, doc0, at = [], [], 0, 0
        start_np = start_t.numpy()
        for bert_batch, abs_lens, idxs in forwards:
            b, max_seq_len = len(abs_lens), max(bert_batch['seq_lens'])
            assert bert_batch['tokid_tt'].shape == (b, max_seq_len)
            tables, _ = span_range_tables([s for s, _ in idxs], [n for _, n in idxs], row_base=start_np[doc0:doc0 + b],
                                          max_seq_len=max_seq_len)
            parts.append(np.stack(tables))
            spans.append((at, at + parts[-1].shape[1]))
            at += parts[-1].shape[1]
            doc0 += b
        flat = torch.from_numpy(np.concatenate(parts, 1) if parts else np.zeros((4, 0), np.int32)).to(dev)

        def fill():
            rows = torch.empty(max(total, 1), 768, device=dev, dtype=torch.float32)[:total]
            for (bert_batch, _, _), (r0, r1) in zip(forwards, spans):
                hidden = enc.forward_hidden(bert_batch['tokid_tt'], token_type_ids=bert_batch['seg_tt'],
                                            attention_mask=bert_batch['attnmask_tt'], check_ids=False)
                ops.span_pool_ranges(hidden, flat[0, r0:r1], flat[1, r0:r1], flat[2, r0:r1], rows=rows, out_row=flat[3, r0:r1])
            return rows
        rows = self.model._checked_fill(fill, total, 'AspireContextNER.encode_to_pool')
        return finish_pool(rows, lens_t, start_t, all_lens, pids, planes), layout

    def encode_to_store(self, papers, pids, store=None, batch_size=32, docs_per_forward=64):
        """Every paper encoded through encode_to_pool (papers prepared batch_size at a time), ONE download of the finished row
        matrix, and a RepStore with one [n_sents + n_valid_entities, 768] block per paper under pids[j] plus its row layout
        (RepStore.add's `layout`: the sentence count and, per sentence, the entity rows the reference's facet filter counts for it --
        filter_valid_entities), so that evaluate.score(..., facet=...) filters a query the way get_faceted_encoding does.
        Returns the RepStore (new, or `store` with the papers added), ready for evaluate.score."""
        papers, pids = list(papers), list(pids)
        check_pid_count(pids, len(papers))
        batches = [self.prepare(papers[i:i + batch_size]) for i in range(0, len(papers), batch_size)]
        pool, layout = self.encode_to_pool(batches, pids=pids, docs_per_forward=docs_per_forward)
        rows = pool.repset.rows.cpu().numpy()
        ner_idxs = [x for item in batches for x in item[3]]

        def blocks():
            r0 = 0
            for paper, (n_sents, _), paper_ners, n_rows in zip(papers, layout, ner_idxs, pool.repset.lens_host):
                try:
                    counts = [len(x) for x in filter_valid_entities(paper['ENTITIES'], [len(x) > 0 for x in paper_ners])]
                except IndexError:          # the reference's filter raises on this paper: so does RepStore.faceted
                    counts = None
                yield rows[r0:r0 + n_rows], (n_sents, counts)
                r0 += n_rows
        return add_to_store(store, pids, blocks())
