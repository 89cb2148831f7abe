"""GPU: the attention kernels on masks that are no prefix, and on trained-checkpoint logits that cross key-tile edges.

include/aspire_hip.h promises `attn_mask != 0 = real token` and HipBertEncoder.__call__ stands in for BertModel(..., attention_mask=...),
but every other encoder test masks a prefix whose first key is real.  The fused kernels (flash_attn_p / p64 / f16x2 / f32) walk the keys in
tiles with a running max: a first tile without one real key -- left padding of a tile or more, real tokens behind the first tile only, an
all-zero row -- is where their mask constant must stay finite, as softmax_mask_kernel's and cls_attn_kernel's does.  Reference: HuggingFace
with EAGER attention on the CPU (scores / 8 (+ bias) + (1 - mask) * finfo.min, soft-max), in float32 and in float64: masked keys weigh
0, a row without a real key attends uniformly over its L keys.

Mask cases, one per row of a batch (at most 8 rows: L = 300 holds ten patterns and takes two batches), L in {40, 130, 300} = one partial
128-key tile, two tiles with a nearly empty second one, three tiles; a pattern that does not fit a length is left out there:
  a prefix (control)   b left padding of 5   c of exactly 64   d of exactly 128   e of 131   f real keys in [0, 100) and [256, 300) only
  g only key L - 1 real   h only key 0 real   i Bernoulli(0.7) holes   j an all-zero row, between valid rows

Second half: heavy_tailed_bert's logits of +-50 at L = 300 and 512, where the running max jumps by tens BETWEEN tiles (the existing heavy
tests stop at L = 128 = one tile), at test_gpu_encoder_heavy.py's bar against float64."""
import copy

import pytest
import torch

from heavy_bert import attention_logit_range, heavy_tailed_bert
from test_gpu_encoder import _batch, _bert
from test_gpu_sbert import _model as _sbert_model

pytestmark = pytest.mark.gpu
TOL = 1e-4               # the encoder suite's bar against HuggingFace fp32 (tests/test_gpu_encoder.py)
FORM_TOL = 2e-5          # fused against the three-kernel form (test_fused_attention_matches_three_kernel_form)
LENGTHS = (40, 130, 300)
# pins -> attention kernel (aspire_amd/csrc/encoder.hip: plan_forward, run_layer)
FORMS = {
    'p': dict(GEMM='planes'),                           # flash_attn_p_kernel
    'p64': dict(GEMM='planes', ATTN='p64'),             # flash_attn_p64_kernel (no biased form)
    'f16x2': dict(GEMM='bf16x3'),                       # flash_attn_f16x2_kernel
    'f32': dict(GEMM='bf16x3', ATTN='f32'),             # flash_attn_f32_kernel
    'gemm': dict(ATTN='gemm'),                          # softmax_mask_kernel between two GEMMs
    'planes-f16x2': dict(GEMM='planes', ATTN='f16x2'),  # flash_attn_f16x2_kernel behind the plane GEMMs: flash_attn_p's bits
}
FUSED = ('p', 'p64', 'f16x2', 'f32')
KIND_FORMS = {'bert': ('p', 'p64', 'f16x2', 'f32', 'gemm'), 'mpnet': ('p', 'f16x2', 'f32', 'gemm'), 'roberta': ('p',)}
PAD = {'bert': 0, 'mpnet': 1, 'roberta': 1}


def _mask_rows(l):
    """{case: int64 [l]} in the order a .. i, then j"""
    def left(n):
        r = torch.ones(l, dtype=torch.long)
        r[:n] = 0
        return r

    def only(*ranges):
        r = torch.zeros(l, dtype=torch.long)
        for lo, hi in ranges:
            r[lo:hi] = 1
        return r
    rows = {'a': only((0, 2 * l // 3)), 'b': left(5)}
    for case, n in (('c', 64), ('d', 128), ('e', 131)):
        if l > n:
            rows[case] = left(n)
    if l == 300:
        rows['f'] = only((0, 100), (256, 300))
    rows['g'] = only((l - 1, l))
    rows['h'] = only((0, 1))
    rows['i'] = (torch.rand(l, generator=torch.Generator().manual_seed(7000 + l)) < 0.7).long()
    rows['j'] = only()
    return rows


def _groups(l):
    """the cases of length l in batches of at most 8 rows; the all-zero row second to last in its batch: the valid document in front
    of it runs its last key tile into the bad document's rows (flash_attn_p), the one behind it starts where those end"""
    names = [c for c in _mask_rows(l) if c != 'j']
    first, rest = ([], names) if len(names) < 8 else (names[:5], names[5:])
    return ([tuple(first)] if first else []) + [tuple(rest[:-1] + ['j'] + rest[-1:])]


BATCHES = [(l, gi) for l in LENGTHS for gi in range(len(_groups(l)))]
J_BATCHES = [(l, gi) for l, gi in BATCHES if 'j' in _groups(l)[gi]]


def _inputs(kind, l, gi, variant='masks'):
    """(cases, ids, mask) of batch gi at length l; ids carry the model's pad id wherever the mask is 0.  variant 'no-j': the all-zero
    row is a fully valid document instead, every other row the same -- the batch WITHOUT the bad document, at the same launch shapes.
    variant 'ids-under-holes' (RoBERTa): one more row, i*, the holes of case i over ids that are NOT pad ids."""
    cases = _groups(l)[gi]
    rows = _mask_rows(l)
    mask = torch.stack([rows[c] for c in cases])
    ids = torch.randint(5, 3000, mask.shape, generator=torch.Generator().manual_seed(7100 + 10 * l + gi))
    if variant == 'no-j':
        mask[cases.index('j')] = 1
    padded = ids * mask + PAD[kind] * (1 - mask)
    if variant == 'ids-under-holes':
        # (one more row; in a batch that has 8 it takes the place of the first one, the control)
        keep = slice(1, None) if len(cases) == 8 else slice(None)
        under = ids[cases.index('i')][None]
        cases = cases[keep] + ('i*',)
        mask = torch.cat([mask[keep], rows['i'][None]])
        padded = torch.cat([padded[keep], under])
    return cases, padded, mask


def _eager(m):
    m.set_attn_implementation('eager')
    assert m.config._attn_implementation == 'eager'
    return m


def _refs(m, ids, mask):
    """HuggingFace on the CPU in float32 and in float64 (tests/test_gpu_encoder_heavy.py: _refs)"""
    with torch.no_grad():
        w32 = m(ids, attention_mask=mask).last_hidden_state
        w64 = m.double()(ids, attention_mask=mask).last_hidden_state
        m.float()
    return w32, w64


class _Runs:
    """models, encoders, references and GPU outputs of this module, each computed once"""

    def __init__(self):
        self.models, self.encoders, self.refs, self.outs = {}, {}, {}, {}

    def model(self, kind):
        if kind not in self.models:
            # (test_gpu_sbert's builders are cached and shared: a copy takes the eager attention)
            self.models[kind] = _eager(_bert(2, seed=61) if kind == 'bert' else copy.deepcopy(_sbert_model(kind)))
        return self.models[kind]

    def encoder(self, kind):
        from aspire_amd.encoder import HipBertEncoder
        if kind not in self.encoders:
            self.encoders[kind] = HipBertEncoder(self.model(kind))
            assert self.encoders[kind]._w.planes
        return self.encoders[kind]

    def ref(self, kind, l, gi, variant='masks'):
        key = (kind, l, gi, variant)
        if key not in self.refs:
            _, ids, mask = _inputs(kind, l, gi, variant)
            w32, w64 = _refs(self.model(kind), ids, mask)
            # the reference itself: finite on every mask, float32 next to float64
            assert torch.isfinite(w32).all() and torch.isfinite(w64).all()
            assert (w32.double() - w64).abs().max().item() < 1e-5, key
            self.refs[key] = (w32, w64)
        return self.refs[key]

    def out(self, kind, form, l, gi, variant='masks'):
        from aspire_amd._lib import pinned
        key = (kind, form, l, gi, variant)
        if key not in self.outs:
            _, ids, mask = _inputs(kind, l, gi, variant)
            enc = self.encoder(kind)
            with pinned(**FORMS[form]):
                self.outs[key] = enc.forward_hidden(ids, None, mask).cpu()
            assert enc.status() == 0
        return self.outs[key]


@pytest.fixture(scope='module')
def runs():
    return _Runs()


def _check_against_transformers(runs, kind, form, l, gi, variant='masks'):
    cases, _, mask = _inputs(kind, l, gi, variant)
    w32, w64 = runs.ref(kind, l, gi, variant)
    got = runs.out(kind, form, l, gi, variant)
    bad = []
    for r, case in enumerate(cases):
        finite = bool(torch.isfinite(got[r]).all())
        err = (got[r] - w32[r]).abs().max().item()          # every position, masked query rows and the all-masked document included
        print(f'MASKS {kind} {form} L={l} case {case}: finite {finite}  max |got - hf32| {err:.3e}  |got - hf64| '
              f'{(got[r].double() - w64[r]).abs().max().item():.3e}  (real keys {int(mask[r].sum())})')
        if not finite or not err < TOL:
            bad.append((case, finite, err))
    assert not bad, (kind, form, l, bad)


def test_the_mask_cases_are_what_they_claim():
    """from the inputs alone: which cases leave the first 128-key (64-key) tile without a real key, and a later tile with one"""
    r = _mask_rows(300)
    assert set(r) == set('abcdefghij') and set(_mask_rows(130)) == set('abcdghij') and set(_mask_rows(40)) == set('abghij')
    first128 = {c for c, m in r.items() if m[:128].sum() == 0}
    first64 = {c for c, m in r.items() if m[:64].sum() == 0}
    assert first128 == {'d', 'e', 'g', 'j'} and first64 == {'c', 'd', 'e', 'g', 'j'}
    assert r['d'][128] == 1 and r['c'][63] == 0 and r['c'][64] == 1 and r['e'][130] == 0 and r['e'][131] == 1
    assert r['f'][128:256].sum() == 0 and r['f'][64:128].sum() > 0 and r['f'][256:].sum() == 44      # a middle tile masked; for p64, 128 .. 255 = two
    assert 0 < r['i'].sum() < 300 and r['j'].sum() == 0 and r['g'].sum() == 1 and r['h'][0] == 1 and r['h'].sum() == 1
    assert _mask_rows(130)['d'].sum() == 2                                # the second tile's two keys are the only real ones
    for l in LENGTHS:
        assert sorted(c for g in _groups(l) for c in g) == sorted(_mask_rows(l)) and all(len(g) <= 8 for g in _groups(l))
        for g in _groups(l):
            if 'j' in g:
                assert 0 < g.index('j') < len(g) - 1


@pytest.mark.parametrize('l,gi', BATCHES)
@pytest.mark.parametrize('form', KIND_FORMS['bert'] + ('planes-f16x2',))
def test_bert_on_mask_patterns_matches_transformers(runs, form, l, gi):
    _check_against_transformers(runs, 'bert', form, l, gi)


@pytest.mark.parametrize('l,gi', BATCHES)
@pytest.mark.parametrize('form', KIND_FORMS['mpnet'] + ('planes-f16x2',))
def test_mpnet_on_mask_patterns_matches_transformers(runs, form, l, gi):
    """the biased instantiations; the bias table is indexed by key - query: left padding and holes weigh entries far from the diagonal"""
    _check_against_transformers(runs, 'mpnet', form, l, gi)


@pytest.mark.parametrize('l,gi', BATCHES)
def test_roberta_on_mask_patterns_takes_position_ids_from_the_ids(runs, l, gi):
    """pad ids wherever the mask is 0, so HF's position ids (from the ids: pad tokens get padding_idx, real ones count on from it)
    skip the holes; and one row whose holes lie over REAL ids: its positions count through the holes -- ids decide, not the mask"""
    from aspire_amd.encoder import position_ids_from_input_ids
    variant = 'ids-under-holes' if 'i' in _groups(l)[gi] else 'masks'
    cases, ids, mask = _inputs('roberta', l, gi, variant)
    pos = position_ids_from_input_ids(ids, 1)
    by_mask = torch.cumsum(mask, 1) * mask + 1
    for r, case in enumerate(cases):
        assert torch.equal(pos[r], by_mask[r]) == (case != 'i*'), case
    m = runs.model('roberta')
    assert torch.equal(m.embeddings.create_position_ids_from_input_ids(ids, 1), pos)
    _check_against_transformers(runs, 'roberta', 'p', l, gi, variant)


@pytest.mark.parametrize('l,gi', J_BATCHES)
@pytest.mark.parametrize('kind,form', [('bert', f) for f in KIND_FORMS['bert']] + [('mpnet', f) for f in KIND_FORMS['mpnet']])
def test_an_all_masked_document_does_not_leak_into_its_neighbours(runs, kind, form, l, gi):
    """the valid documents of the batch that holds the all-zero row have the bits they have in the same batch without it (that row a
    fully valid document instead: the same launches).  Two layers: whatever the bad document's rows hold after layer 1 is what the
    neighbour's last key tile runs into in layer 2 (flash_attn_p_kernel: weighted exactly 0)."""
    cases = _groups(l)[gi]
    with_j, without = runs.out(kind, form, l, gi), runs.out(kind, form, l, gi, 'no-j')
    assert torch.isfinite(with_j).all()
    for r, case in enumerate(cases):
        if case != 'j':
            assert torch.equal(with_j[r], without[r]), (case, (with_j[r] - without[r]).abs().max().item())
    assert not torch.equal(with_j[cases.index('j')], without[cases.index('j')])


@pytest.mark.parametrize('l,gi', BATCHES)
@pytest.mark.parametrize('kind', ['bert', 'mpnet'])
def test_plane_attention_has_the_f16x2_bits_on_mask_patterns(runs, kind, l, gi):
    """test_gpu_attn_planes.py's contract (the same bits at every length) on these masks"""
    new, old = runs.out(kind, 'p', l, gi), runs.out(kind, 'planes-f16x2', l, gi)
    assert torch.isfinite(new).all()
    assert torch.equal(new, old), (new - old).abs().max().item()


@pytest.mark.parametrize('l,gi', BATCHES)
@pytest.mark.parametrize('kind,form', [('bert', f) for f in FUSED] + [('mpnet', f) for f in FUSED if f != 'p64'])
def test_fused_attention_matches_the_three_kernel_form_on_mask_patterns(runs, kind, form, l, gi):
    fused, ref = runs.out(kind, form, l, gi), runs.out(kind, 'gemm', l, gi)
    assert torch.isfinite(fused).all() and torch.isfinite(ref).all()
    d = (fused - ref).abs().amax((1, 2))
    print(f'MASKS {kind} {form} against gemm L={l}: ' + '  '.join(f'{c} {x:.2e}' for c, x in zip(_groups(l)[gi], d.tolist())))
    assert d.max().item() < FORM_TOL, (kind, form, l, d.tolist())


@pytest.mark.parametrize('l,gi', BATCHES)
@pytest.mark.parametrize('gemm', ['bf16x3', 'planes'])
def test_forward_cls_on_mask_patterns(runs, gemm, l, gi):
    """aspire_bert_forward_cls_f32 on the 2-layer model: full attention in the lower layer, cls_attn_kernel in the last one, on the fp32
    qkv (bf16x3) and on the fp16 planes"""
    from aspire_amd._lib import pinned
    cases, ids, mask = _inputs('bert', l, gi)
    want = runs.ref('bert', l, gi)[0][:, 0]
    enc = runs.encoder('bert')
    with pinned(GEMM=gemm):
        got = enc.forward_cls(ids, None, mask)[0].cpu()
    assert enc.status() == 0
    err = (got - want).abs().amax(1)
    print(f'MASKS forward_cls {gemm} L={l}: ' + '  '.join(f'{c} {x:.2e}' for c, x in zip(cases, err.tolist())))
    assert torch.isfinite(got).all(), [c for c, row in zip(cases, got) if not torch.isfinite(row).all()]
    assert err.max().item() < TOL, (gemm, l, list(zip(cases, err.tolist())))


# ---- logits of +-50 across key tiles ------------------------------------------------------------------------------------------------
HEAVY_BATCHES = ('4x300', '3x512', '4x300-masks')
SCALED_HEADS_LAYER0 = (0, 5, 7, 10)          # tests/heavy_bert.py: the heads whose query / key projections layer 0 scales up


def _heavy_inputs(name):
    if name == '4x300':
        return _batch(4, 300, 3000, seed=31)[:3]
    if name == '3x512':
        return _batch(3, 512, 3000, seed=37)[:3]
    tok, seg, mask, _ = _batch(4, 300, 3000, seed=41)
    rows = _mask_rows(300)
    mask[1], mask[2] = rows['e'], rows['i']             # left padding of 131, holes; rows 0 and 3 keep their prefixes
    return torch.where(mask.bool(), tok.clamp_min(5), torch.zeros_like(tok)), seg, mask


def _late_max_fraction(m, tok, seg, mask):
    """over the (document, scaled head, real query) triples of layer 0: how often the largest real-key logit lies outside keys 0 .. 127"""
    with torch.no_grad():
        hs = m(tok, token_type_ids=seg, attention_mask=mask, output_hidden_states=True).hidden_states[0]
        att = m.encoder.layer[0].attention.self
        b, l, _ = hs.shape
        q = att.query(hs).view(b, l, 12, 64).transpose(1, 2)[:, list(SCALED_HEADS_LAYER0)]
        k = att.key(hs).view(b, l, 12, 64).transpose(1, 2)[:, list(SCALED_HEADS_LAYER0)]
        s = ((q @ k.transpose(-1, -2)) / 8.0).masked_fill(~mask.bool()[:, None, None, :], float('-inf'))
        late = s.argmax(-1) >= 128
        real_q = mask.bool()[:, None, :].expand_as(late)
        return float((late & real_q).sum()) / float(real_q.sum())


@pytest.fixture(scope='module')
def heavy():
    m = _eager(heavy_tailed_bert(2, seed=2))
    refs = {}
    for name in HEAVY_BATCHES:
        tok, seg, mask = _heavy_inputs(name)
        with torch.no_grad():
            w32 = m(tok, token_type_ids=seg, attention_mask=mask).last_hidden_state
            w64 = m.double()(tok, token_type_ids=seg, attention_mask=mask).last_hidden_state
            m.float()
        refs[name] = (tok, seg, mask, w32, w64)
    return m, refs, {}


@pytest.mark.parametrize('name', HEAVY_BATCHES)
def test_heavy_batches_have_large_logits_whose_maximum_moves_to_a_later_tile(heavy, name):
    """from the reference alone: the model is calibrated on 4 x 96; at these lengths layer 0 still has logits beyond +-30, and for at
    least a quarter of the queries of the scaled heads the largest real-key logit sits behind the first 128-key tile, so the running
    max does jump upward in a later tile"""
    m, refs, _ = heavy
    tok, seg, mask, w32, w64 = refs[name]
    lo, hi = attention_logit_range(m, tok, seg, mask, 0)
    frac = _late_max_fraction(m, tok, seg, mask)
    print(f'HEAVY {name}: layer-0 logits {lo:.1f} .. {hi:.1f}; the maximum lies behind key 127 for {frac:.3f} of the scaled heads\' queries')
    assert lo < -30 and hi > 30, (lo, hi)
    assert frac >= 0.25, frac
    assert torch.isfinite(w32).all() and torch.isfinite(w64).all()


@pytest.mark.parametrize('name', HEAVY_BATCHES)
@pytest.mark.parametrize('form', ['p', 'p64', 'f16x2', 'f32', 'gemm'])
def test_heavy_tailed_logits_across_key_tiles(heavy, form, name):
    """test_gpu_encoder_heavy.py's bar: against float64 no further than max(1e-4, 1.5 x HuggingFace fp32's own distance from float64)
    over the real positions, and within twice that of the fp32 reference"""
    from aspire_amd._lib import pinned
    from aspire_amd.encoder import HipBertEncoder
    m, refs, cache = heavy
    tok, seg, mask, w32, w64 = refs[name]
    if 'enc' not in cache:
        cache['enc'] = HipBertEncoder(m)
    enc = cache['enc']
    assert enc._w.planes, 'the weights must fit the fp16 planes (|w| <= 1023): no silent bf16x3 path'
    with pinned(**FORMS[form]):
        got = enc.forward_hidden(tok, seg, mask).cpu()
    assert enc.status() == 0
    real = mask.bool()
    ref_err = (w32.double() - w64)[real].abs().max().item()
    err = (got.double() - w64)[real].abs().max().item()
    bar = max(1e-4, 1.5 * ref_err)
    print(f'HEAVY {name} {form}: |got - hf64| {err:.3e}  |hf32 - hf64| {ref_err:.3e}  bar {bar:.3e}  |got - hf32| {(got - w32)[real].abs().max().item():.3e}')
    assert torch.isfinite(got).all()
    assert err <= bar, (err, ref_err)
    assert (got - w32)[real].abs().max().item() <= 2 * bar
