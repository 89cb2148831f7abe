"""A0: batch preparation for the contextual sentence encoder (host side, integer only).

Same contract as the reference's ``prepare_abstracts`` / ``prepare_bert_sentences``
(examples/ex_aspire_consent.py:107-212; originals src/learning/batchers.py:525-630):

  * sentence 0 of every document is ``TITLE + ' [SEP] '``; its token positions are NOT returned
  * positions count from 1 (position 0 is [CLS])
  * at most 500 word pieces per document: the sentence that crosses the cap is kept only up to the cap
    (dropped entirely if nothing of it fits) and everything after it is discarded
  * ids / segment ids / attention mask are right-padded with ``tokenizer.pad_token_id``

Besides the reference's return values, ``spans_to_csr`` flattens the ragged index lists into the
(tok_idx, span_off) arrays aspire_span_mean_pool_f32 consumes, and ``span_range_tables`` turns sentence and entity spans into
the (document, first token, token count) rows aspire_span_pool_ranges_f32 consumes (the contextual-entity model,
aspire_amd/contextner.py).
"""
import re

import numpy as np
import torch

MAX_NUM_TOKS = 500


def _with_special_tokens(tokenizer, ids):
    # transformers 4.5.1 (the reference's pin) has build_inputs_with_special_tokens; transformers >= 5
    # removed it from BertTokenizer.  For a single sequence both mean [CLS] ids [SEP].
    build = getattr(tokenizer, 'build_inputs_with_special_tokens', None)
    if build is not None:
        return build(token_ids_0=ids)
    return [tokenizer.cls_token_id] + ids + [tokenizer.sep_token_id]


def _word_pieces(tokenizer, sents, want_text=True):
    """tokenizer.tokenize + convert_tokens_to_ids of every sentence (ex_aspire_consent.py:135-137), as (pieces, ids) per sentence.
    A fast (Rust) tokenizer takes all the sentences of the batch in ONE call -- the same encode its tokenize() runs per sentence --
    instead of one Python round trip each: the reference's loop prepares ~700 documents/s per core, a ninth of what one GPU encodes."""
    if getattr(tokenizer, 'is_fast', False) and sents:
        ids = tokenizer(list(sents), add_special_tokens=False, return_attention_mask=False, return_token_type_ids=False,
                        verbose=False)['input_ids']
        # (the word-piece strings only where the caller returns them: prepare_abstracts does not)
        return [(tokenizer.convert_ids_to_tokens(x) if want_text else x, list(x)) for x in ids]
    out = []
    for sent in sents:
        pieces = tokenizer.tokenize(sent)
        out.append((pieces, tokenizer.convert_tokens_to_ids(pieces)))
    return out


def prepare_bert_sentences(batch_doc_sents, tokenizer, want_text=True, tokenized=None):
    """
    :param batch_doc_sents: list(list(string)); per document: title sentence then abstract sentences.
    :param want_text: False: batch_tokenized_text comes back as ids instead of word-piece strings (prepare_abstracts drops it).
    :param tokenized: _word_pieces' output for the sentences of all documents in order, where the caller has it already
        (prepare_abstracts_entities matches the entities against the same tokenisation); None: tokenised here.
    :return: bert_batch dict('tokid_tt', 'seg_tt', 'attnmask_tt', 'seq_lens'),
             batch_tokenized_text list(list(string)),
             batch_sent_token_idxs list(list(list(int))) -- title excluded.
    """
    docs_ids, docs_text, docs_spans = [], [], []
    if tokenized is None:
        tokenized = _word_pieces(tokenizer, [sent for doc_sents in batch_doc_sents for sent in doc_sents], want_text)
    tokenized = iter(tokenized)
    for doc_sents in batch_doc_sents:
        ids, text, spans = [], [], []
        used = 0
        doc_pieces = [next(tokenized) for _ in doc_sents]
        for pieces, piece_ids in doc_pieces:
            room = MAX_NUM_TOKS - used
            keep = min(len(pieces), room)
            overflow = len(pieces) > room
            if keep > 0 or not overflow:
                # (an empty sentence that fits still gets its empty span, like the reference)
                spans.append(list(range(used + 1, used + 1 + keep)))
                text.extend(pieces[:keep])
                ids.extend(piece_ids[:keep])
            if overflow:
                break
            used += keep
        docs_text.append(text)
        docs_spans.append(spans[1:])
        docs_ids.append(_with_special_tokens(tokenizer, ids))
    seq_lens = [len(x) for x in docs_ids]
    max_seq_len = max(seq_lens) if seq_lens else 0
    pad = tokenizer.pad_token_id
    tok, seg, att = [], [], []
    for ids in docs_ids:
        n_pad = max_seq_len - len(ids)
        tok.append(ids + [pad] * n_pad)
        seg.append([0] * len(ids) + [pad] * n_pad)
        att.append([1] * len(ids) + [pad] * n_pad)
    bert_batch = {'tokid_tt': torch.tensor(tok), 'seg_tt': torch.tensor(seg), 'attnmask_tt': torch.tensor(att),
                  'seq_lens': seq_lens}
    return bert_batch, docs_text, docs_spans


def prepare_abstracts(batch_abs, pt_lm_tokenizer):
    """
    :param batch_abs: list(dict) with 'TITLE' (str) and 'ABSTRACT' (list of sentence strings).
    :return: bert_batch, abs_lens list(int), sent_token_idxs list(list(list(int)))
    """
    batch_abs_seqs = [[ex_abs['TITLE'] + ' [SEP] '] + list(ex_abs['ABSTRACT']) for ex_abs in batch_abs]
    bert_batch, _, sent_token_idxs = prepare_bert_sentences(batch_doc_sents=batch_abs_seqs, tokenizer=pt_lm_tokenizer, want_text=False)
    abs_lens = []
    for abs_sent_tok_idxs in sent_token_idxs:
        num_sents = len(abs_sent_tok_idxs)
        abs_lens.append(num_sents)
        assert (num_sents > 0)   # ex_aspire_consent.py:210
    return bert_batch, abs_lens, sent_token_idxs


ALIGN_TYPES = ('cc_align', 'abs_align')     # AbsSentTokBatcherPreAlign.align_type (batchers.py:639-640)


def _prepare_abstracts_align(batch_abs, pt_lm_tokenizer, align_type):
    """AbsSentTokBatcherPreAlign.prepare_abstracts (batchers.py:710-746): prepare_abstracts and the examples' pre-computed
    alignments [query sentence, candidate sentence] (copies), None when no example carries `align_type`."""
    align = []
    for ex_abs in batch_abs:
        if align_type in ex_abs:
            assert (len(ex_abs[align_type]) == 2)   # batchers.py:729
            align.append(list(ex_abs[align_type]))
    bert_batch, abs_lens, sent_token_idxs = prepare_abstracts(batch_abs, pt_lm_tokenizer)
    if align:
        assert (len(align) == len(abs_lens))   # batchers.py:743: every example carries the key, or none
    return bert_batch, abs_lens, sent_token_idxs, align or None


def make_batch(raw_feed, pt_lm_tokenizer, align_type='cc_align'):
    """AbsSentTokBatcher.make_batch and AbsSentTokBatcherPreAlign.make_batch (batchers.py:462-523, :642-746) in one: the batch dict
    of RankLoss / SupAlignRankLoss.forward_rank from a raw feed of example dicts ('TITLE', 'ABSTRACT' and, pre-aligned, `align_type`).
      'query_texts', 'pos_texts' and 'neg_texts' (the dev set): query_ / pos_ / neg_ + bert_batch, abs_lens, senttok_idxs
      'query_texts' and 'pos_texts' (training with in-batch negatives): query_ / pos_
      'query_texts' alone (encoding): bert_batch, abs_lens, senttok_idxs
    'pos_align_idxs' / 'neg_align_idxs' are present exactly when every example of that side carries `align_type` ('cc_align' or
    'abs_align'); when only some do, the reference's assertion fires.  The alignment lists are copies of the examples'."""
    if align_type not in ALIGN_TYPES:
        raise ValueError(f'Unknown align_type: {align_type}')
    qbert_batch, qabs_len, qabs_senttok_idxs = prepare_abstracts(raw_feed['query_texts'], pt_lm_tokenizer)
    if 'pos_texts' not in raw_feed:     # Happens when the function is called from other scripts to encode text.
        return {'bert_batch': qbert_batch, 'abs_lens': qabs_len, 'senttok_idxs': qabs_senttok_idxs}
    batch_dict = {'query_bert_batch': qbert_batch, 'query_abs_lens': qabs_len, 'query_senttok_idxs': qabs_senttok_idxs}
    sides = ('neg', 'pos') if 'neg_texts' in raw_feed else ('pos',)      # (the reference's order: negatives first in the dev set)
    for side in sides:
        bert_batch, abs_len, senttok_idxs, align = _prepare_abstracts_align(raw_feed[side + '_texts'], pt_lm_tokenizer, align_type)
        batch_dict.update({side + '_bert_batch': bert_batch, side + '_abs_lens': abs_len, side + '_senttok_idxs': senttok_idxs})
        if align is not None:
            batch_dict[side + '_align_idxs'] = align
    return batch_dict


def spans_to_csr(batch_senttok_idxs, max_sents):
    """Ragged [B][<=S][tokens] position lists -> (tok_idx int32 [N], span_off int32 [B*S+1]) on the host.
    Slots beyond a document's sentence count are empty (they pool to exact zeros)."""
    flat, off = [], [0]
    for doc in batch_senttok_idxs:
        for s in range(max_sents):
            if s < len(doc):
                flat.extend(doc[s])
            off.append(len(flat))
    return (torch.tensor(flat if flat else [0], dtype=torch.int32)[:len(flat)].contiguous(),
            torch.tensor(off, dtype=torch.int32))


# ---- the contextual-entity model's inputs (aspire_amd/contextner.py): sentence spans + one span per named entity ----------------
def find_sublist_range(suplist, sublist):
    """AspireContextNER.find_sublist_range (src/evaluation/utils/models.py:684-697): the positions of the FIRST occurrence of
    sublist inside suplist as a list of consecutive ints, None when there is none ([] for an empty sublist of a non-empty suplist)."""
    n, m = len(suplist), len(sublist)
    for i in range(n):
        if i + m <= n and suplist[i:i + m] == sublist:
            return list(range(i, i + m))
    return None


def _ner_token_idxs(batch_papers, sent_token_idxs, sent_ids, ner_ids):
    """ner_token_idxs on word-piece ids: sent_ids[d][i] the ids of ABSTRACT sentence i of paper d (at least the kept ones), ner_ids an
    iterator over the ids of the entities of the kept sentences in paper / sentence / entity order."""
    out = []
    for paper, paper_sent_idxs, paper_sent_ids in zip(batch_papers, sent_token_idxs, sent_ids):
        paper_out = []
        # (zip: the entities of sentences beyond the kept ones -- dropped by the 500-piece cap -- get NO entry, models.py:668)
        for ners, tokens, token_idxs in zip(paper['ENTITIES'], paper_sent_ids, paper_sent_idxs):
            tokens = list(tokens)
            for _ in ners:
                ner_range = find_sublist_range(tokens, list(next(ner_ids)))
                # only an entity wholly inside what the cap kept of its sentence has token positions (models.py:674-679)
                if ner_range and ner_range[-1] < len(token_idxs):
                    paper_out.append([token_idxs[i] for i in ner_range])
                else:
                    paper_out.append([])
        out.append(paper_out)
    return out


def _kept_entities(batch_papers, sent_token_idxs):
    return [ner for paper, idxs in zip(batch_papers, sent_token_idxs)
            for ners, _, _ in zip(paper['ENTITIES'], paper['ABSTRACT'], idxs) for ner in ners]


def ner_token_idxs(batch_papers, sent_token_idxs, tokenizer):
    """AspireContextNER._get_ner_token_idxs (models.py:649-682): per paper one entry per entity of its kept sentences (ENTITIES[i]
    are the entity strings of ABSTRACT[i]), in order: the token positions of the entity's first occurrence in its sentence's own
    tokenisation, or [] when its word pieces are not found there or reach into the part of the sentence the 500-piece cap cut.
    Pieces are compared as vocabulary ids (a word piece and its id name each other; both sides go through the same tokenizer)."""
    sents = [list(paper['ABSTRACT'])[:len(idxs)] for paper, idxs in zip(batch_papers, sent_token_idxs)]
    pieces = iter(_word_pieces(tokenizer, [s for doc in sents for s in doc], want_text=False))
    sent_ids = [[next(pieces)[1] for _ in doc] for doc in sents]
    ner_ids = (ids for _, ids in _word_pieces(tokenizer, _kept_entities(batch_papers, sent_token_idxs), want_text=False))
    return _ner_token_idxs(batch_papers, sent_token_idxs, sent_ids, ner_ids)


def prepare_abstracts_entities(batch_abs, tokenizer):
    """AspireContextNER._preprocess_input (models.py:641-647): prepare_abstracts plus the entities' token positions.  Every
    sentence is tokenised ONCE (one batched call with a fast tokenizer) for both; the entities in one more call.
    :param batch_abs: list(dict) with 'TITLE', 'ABSTRACT' (list of sentences) and 'ENTITIES' (per sentence a list of strings).
    :return: bert_batch, abs_lens, sent_token_idxs, ner_token_idxs"""
    batch_abs_seqs = [[ex_abs['TITLE'] + ' [SEP] '] + list(ex_abs['ABSTRACT']) for ex_abs in batch_abs]
    tokenized = _word_pieces(tokenizer, [sent for doc_sents in batch_abs_seqs for sent in doc_sents], want_text=False)
    bert_batch, _, sent_token_idxs = prepare_bert_sentences(batch_abs_seqs, tokenizer, want_text=False, tokenized=tokenized)
    abs_lens = [len(x) for x in sent_token_idxs]
    assert all(n > 0 for n in abs_lens)   # ex_aspire_consent.py:210
    sent_ids, at = [], 0
    for doc_sents in batch_abs_seqs:
        sent_ids.append([ids for _, ids in tokenized[at + 1:at + len(doc_sents)]])      # (the title is no entity sentence)
        at += len(doc_sents)
    ner_ids = (ids for _, ids in _word_pieces(tokenizer, _kept_entities(batch_abs, sent_token_idxs), want_text=False))
    return bert_batch, abs_lens, sent_token_idxs, _ner_token_idxs(batch_abs, sent_token_idxs, sent_ids, ner_ids)


def append_entities(batch_papers):
    """AspireNER._append_entities (models.py:224-233): every paper's entity strings appended to its abstract as further sentences."""
    return [{'TITLE': paper['TITLE'], 'ABSTRACT': list(paper['ABSTRACT']) + [ner for ners in paper['ENTITIES'] for ner in ners]}
            for paper in batch_papers]


def span_range_tables(sent_token_idxs, ner_token_idxs, row_base=None, pad_sents=None, max_seq_len=None):
    """The rows aspire_span_pool_ranges_f32 pools, document by document: a document's sentence spans, then its NON-EMPTY entity
    spans (the reference drops the empty ones at models.py:636).  Every span must be a run of consecutive positions (sentence
    spans are: SURVEY.md section 8 A0; entity spans are: find_sublist_range), else ValueError; an empty sentence span is a row of
    length 0 (exact zeros).
    :param row_base: per document the row of a rows + CSR store where its rows begin -> out_row; None: out_row is None (row r).
    :param pad_sents: every document's sentence rows filled up to this many with zero-length rows (the padded [B, S, 768] form).
    :param max_seq_len: positions outside [0, max_seq_len) raise IndexError (as fancy indexing does on the reference path).
    :return: (doc, tok_start, tok_len, out_row) int32 numpy arrays [R] and n_entities, the valid-entity count per document."""
    doc, start, length, out_row, n_entities = [], [], [], [], []
    for d, sents in enumerate(sent_token_idxs):
        ners = [x for x in (ner_token_idxs[d] if ner_token_idxs is not None else []) if len(x) > 0]
        spans = [list(x) for x in sents]
        if pad_sents is not None:
            spans += [[] for _ in range(pad_sents - len(spans))]
        spans += [list(x) for x in ners]
        for k, span in enumerate(spans):
            n = len(span)
            if n and span != list(range(span[0], span[0] + n)):
                raise ValueError(f'document {d}: span {span} is not a run of consecutive token positions')
            if n and max_seq_len is not None and (span[0] < 0 or span[-1] >= max_seq_len):
                raise IndexError('span token index out of range')
            doc.append(d)
            start.append(span[0] if n else 0)
            length.append(n)
            if row_base is not None:
                out_row.append(int(row_base[d]) + k)
        n_entities.append(len(ners))
    as_i32 = lambda x: np.asarray(x, dtype=np.int32)
    return (as_i32(doc), as_i32(start), as_i32(length), as_i32(out_row) if row_base is not None else None), n_entities


# ---- the SPECTER-CoCite bi-encoder's inputs (aspire_amd/bienc.py): one whole-abstract sequence per document --------------------
_SEP_RE = re.compile(r'\[SEP\]')


def batch_tensors(bert_batch):
    """(ids, token type ids or None, attention mask or None) of the README's HF tokenizer dict (input_ids / token_type_ids /
    attention_mask) or of the batchers' (tokid_tt / seg_tt / attnmask_tt)."""
    if 'input_ids' in bert_batch:
        return bert_batch['input_ids'], bert_batch.get('token_type_ids'), bert_batch.get('attention_mask')
    return bert_batch['tokid_tt'], bert_batch.get('seg_tt'), bert_batch.get('attnmask_tt')


def prepare_bert_seqs(sents, tokenizer):
    """SentTripleBatcher.prepare_bert_sentences (src/learning/batchers.py:209-254): every string is ONE sequence, cut to its
    first 500 word pieces, [CLS] ids [SEP]; ids, segment ids and attention mask right-padded with ``tokenizer.pad_token_id``.
    :return: bert_batch dict('tokid_tt', 'seg_tt', 'attnmask_tt', 'seq_lens'), tokenized_text list(list(str)),
             tokenized_batch list(list(int)) (the padded ids)."""
    tokenized_text, tokenized_batch = [], []
    for pieces, piece_ids in _word_pieces(tokenizer, list(sents)):
        tokenized_text.append(pieces[:MAX_NUM_TOKS])
        tokenized_batch.append(_with_special_tokens(tokenizer, piece_ids[:MAX_NUM_TOKS]))
    seq_lens = [len(x) for x in tokenized_batch]
    max_seq_len = max(seq_lens) if seq_lens else -1
    pad = tokenizer.pad_token_id
    seg, att = [], []
    for ids in tokenized_batch:
        n_pad = max_seq_len - len(ids)
        seg.append([0] * len(ids) + [pad] * n_pad)
        att.append([1] * len(ids) + [pad] * n_pad)
        ids.extend([pad] * n_pad)
    bert_batch = {'tokid_tt': torch.tensor(tokenized_batch), 'seg_tt': torch.tensor(seg), 'attnmask_tt': torch.tensor(att),
                  'seq_lens': seq_lens}
    return bert_batch, tokenized_text, tokenized_batch


def prepare_abstract_seqs(batch_abs, pt_lm_tokenizer):
    """AbsTripleBatcher.prepare_abstracts (src/learning/batchers.py:303-321): title and sentences, each with any literal
    '[SEP]' removed, joined by ' [SEP] ' into one sequence per document.  :return: bert_batch (prepare_bert_seqs)."""
    seqs = [' [SEP] '.join(_SEP_RE.sub('', s) for s in [ex_abs['TITLE']] + list(ex_abs['ABSTRACT'])) for ex_abs in batch_abs]
    return prepare_bert_seqs(seqs, pt_lm_tokenizer)[0]


def prepare_eval_seqs(batch_papers, tokenizer):
    """TrainedAbstractModel.encode's input (src/evaluation/utils/models.py:557-563): TITLE + ' [SEP] ' + ' '.join(ABSTRACT), no
    '[SEP]' removal.  :return: bert_batch (prepare_bert_seqs)."""
    return prepare_bert_seqs([p['TITLE'] + ' [SEP] ' + ' '.join(p['ABSTRACT']) for p in batch_papers], tokenizer)[0]


def prepare_eval_ner_seqs(batch_papers, tokenizer):
    """BertNER._pre_process_input_batch (src/evaluation/utils/models.py:368-376): prepare_eval_seqs' text + ' ' + the entity strings
    of all sentences, in order, joined by '. ' + '.'; a paper without entities still gets the trailing ' .'.
    :return: bert_batch (prepare_bert_seqs)."""
    seqs = [p['TITLE'] + ' [SEP] ' + ' '.join(p['ABSTRACT']) + ' ' + '. '.join(ner for ners in p['ENTITIES'] for ner in ners) + '.'
            for p in batch_papers]
    return prepare_bert_seqs(seqs, tokenizer)[0]


# ---- the cosentbert / ictsentbert sentence encoder's inputs (aspire_amd/sentenc.py): one sequence per sentence ------------------
def prepare_sentence_batch(sents, tokenizer, max_seq_length=512):
    """The tokenisation of SentenceTransformer.encode with models.Transformer(max_seq_length=512) (TrainedSentModel,
    src/evaluation/utils/models.py:568-604; recalled from sentence-transformers, which the reference imports): every text
    ``.strip()``ed, then ``tokenizer(texts, padding=True, truncation='longest_first', max_length=max_seq_length,
    return_tensors='pt')``.  :return: the HF dict (input_ids, token_type_ids, attention_mask), right-padded to the longest."""
    return tokenizer([str(s).strip() for s in sents], padding=True, truncation='longest_first', max_length=max_seq_length,
                     return_tensors='pt')


def sentence_buckets(n_tokens, max_tokens=16384):
    """Encoder calls for sentences of n_tokens[i] word pieces each (specials included): the sentences sorted by length
    (stable) and cut into consecutive runs whose padded size, run length x longest member, stays within max_tokens rows (a
    single sentence longer than that is a run of its own).  Returns a list of index arrays into n_tokens: together a
    permutation of range(len(n_tokens))."""
    n_tokens = np.asarray(n_tokens, dtype=np.int64)
    order = np.argsort(n_tokens, kind='stable')
    runs, lo = [], 0
    for i in range(1, len(order) + 1):
        if i == len(order) or (i + 1 - lo) * int(n_tokens[order[i]]) > max_tokens:
            runs.append(order[lo:i])
            lo = i
    return runs


def tokenize_sentences(sents, tokenizer, max_seq_length=512):
    """prepare_sentence_batch's tokenizer call without the padding: (input id lists, token type id lists), one per sentence."""
    enc = tokenizer([str(s).strip() for s in sents], padding=False, truncation='longest_first', max_length=max_seq_length)
    return enc['input_ids'], enc['token_type_ids']


def pad_sentences(ids, types, idx, pad_id):
    """The sentences idx of tokenize_sentences' lists, right-padded to the longest of them as the tokenizer's padding=True pads
    (ids with pad_id, token types and attention mask with 0): int64 (input_ids, token_type_ids, attention_mask) [len(idx), L]."""
    idx = list(idx)
    L = max(len(ids[i]) for i in idx)
    tok = np.full((len(idx), L), pad_id, dtype=np.int64)
    typ = np.zeros((len(idx), L), dtype=np.int64)
    msk = np.zeros((len(idx), L), dtype=np.int64)
    for r, i in enumerate(idx):
        n = len(ids[i])
        tok[r, :n] = ids[i]
        typ[r, :n] = types[i]
        msk[r, :n] = 1
    return torch.from_numpy(tok), torch.from_numpy(typ), torch.from_numpy(msk)
