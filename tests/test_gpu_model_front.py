"""GPU side of aspire_amd/model_front.py's bucketed sentence encode: AspireSentEnc.encode, SentenceModel._encode_sentences and
SimCSE._encode_sentences return, row for row, the bits of a direct HipBertEncoder read-out on the padded run the sentence belongs to.
Seven sentences of 3, 3, 9, 17, 4, 48 and 2 tokens in a budget of 40 token rows: three encoder calls, the longest sentence alone --
the smallest shape at which a wrong pad id, a wrong scatter index or a missing normalize shows."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
N_TOKENS = [3, 3, 9, 17, 4, 48, 2]
MAX_TOKENS = 40
CLS, SEP = 2, 3
SENTS = [f's{i}' for i in range(len(N_TOKENS))]


class _IdTokenizer:
    """The sentence 's<i>' is the id list TABLE[i] ([CLS] ... [SEP]), in each of the three forms the classes ask a tokenizer for."""
    cls_token_id, sep_token_id = CLS, SEP

    def __init__(self, pad):
        g = torch.Generator().manual_seed(9)
        self.pad_token_id = pad
        self.table = {s: [CLS] + torch.randint(4, 64, (n - 2,), generator=g).tolist() + [SEP] for s, n in zip(SENTS, N_TOKENS)}

    def __call__(self, text, **kw):
        if isinstance(text, str):                                    # SentenceModel: one string
            return {'input_ids': list(self.table[text])}
        ids = [list(self.table[t]) for t in text]                    # batch_prep.tokenize_sentences: a list, no padding
        return {'input_ids': ids, 'token_type_ids': [[0] * len(x) for x in ids]}

    def tokenize(self, sent):                                        # batch_prep._word_pieces: pieces, then their ids
        return self.table[sent][1:-1]

    def convert_tokens_to_ids(self, pieces):
        return list(pieces)


def _model(kind):
    """2 layers at BERT-base width, vocabulary 64, 80 positions, random init with LayerNorms and biases perturbed."""
    from transformers import BertConfig, BertModel, RobertaConfig, RobertaModel
    torch.manual_seed({'bert': 31, 'pooled': 32, 'roberta': 33}[kind])
    kw = dict(vocab_size=64, hidden_size=768, num_hidden_layers=2, num_attention_heads=12, intermediate_size=3072,
              max_position_embeddings=80)
    if kind == 'roberta':
        m = RobertaModel(RobertaConfig(type_vocab_size=1, layer_norm_eps=1e-5, pad_token_id=1, **kw), add_pooling_layer=False)
    else:
        m = BertModel(BertConfig(**kw), add_pooling_layer=kind == 'pooled')
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'LayerNorm' in n or n.endswith('.bias'):
                p.add_(0.1 * torch.randn_like(p))
    return m.eval()


@functools.lru_cache(maxsize=None)
def _case(which):
    """(the class's [7, 768] reps on the CPU, the tokenizer, the direct read-out of a padded run)."""
    if which == 'sentenc':
        from aspire_amd.sentenc import AspireSentEnc
        tok = _IdTokenizer(pad=0)
        model = AspireSentEnc(bert_model=_model('bert'), tokenizer=tok, max_seq_length=64)
        got = torch.from_numpy(model.encode(SENTS, max_tokens=MAX_TOKENS))
        return got, tok, lambda *run: model.bert_encoder.forward_cls(*run)[0]
    if which == 'sbert':
        from aspire_amd.sbert import SentenceModel
        tok = _IdTokenizer(pad=1)                                    # RoBERTa pads with id 1: the position ids are told from it
        model = SentenceModel('sbrobertanli', model=_model('roberta'), tokenizer=tok, max_seq_length=64, normalize=True)
        got = torch.from_numpy(model._encode_sentences(SENTS, max_tokens=MAX_TOKENS))
        return got, tok, lambda *run: model.bert_encoder.forward_mean(*run, normalize=True)
    from aspire_amd.baselines import SimCSE
    tok = _IdTokenizer(pad=0)
    model = SimCSE(bert_model=_model('pooled'), tokenizer=tok)
    got = torch.from_numpy(model._encode_sentences(SENTS, max_tokens=MAX_TOKENS))
    return got, tok, lambda *run: model.bert_encoder.forward_pooled(*run)[1]


@pytest.mark.parametrize('which', ['sentenc', 'sbert', 'simcse'])
def test_bucketed_encode_is_the_direct_read_out_of_each_run(which):
    from aspire_amd.batch_prep import pad_sentences, sentence_buckets
    runs = sentence_buckets(N_TOKENS, MAX_TOKENS)
    assert len(runs) == 3 and [N_TOKENS[i] for i in runs[-1]] == [48]
    assert sorted(int(i) for run in runs for i in run) == list(range(len(N_TOKENS)))
    got, tok, read = _case(which)
    assert got.shape == (len(N_TOKENS), 768) and got.dtype == torch.float32
    ids = [tok.table[s] for s in SENTS]
    types = [[0] * len(x) for x in ids]
    for run in runs:
        padded = pad_sentences(ids, types, run, tok.pad_token_id)
        assert padded[0].shape == (len(run), max(N_TOKENS[i] for i in run))
        want = read(*padded).cpu()
        for row, i in enumerate(run):
            assert torch.equal(got[i], want[row]), (which, int(i))
    if which == 'sbert':                                             # normalize=True reached the read-out
        assert float((got.norm(dim=1) - 1).abs().max()) < 1e-5
