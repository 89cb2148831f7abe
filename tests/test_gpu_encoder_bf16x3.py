"""GPU: the training encoder's bf16x3 matmul mode -- aspire_amd.HipBertTrainEncoder(bert, matmul='bf16x3') (torch.ops.aspire.
bert_layers_train_prec / bert_layers_train_cls_prec with ASPIRE_MATMUL_BF16X3): the products with a k-major operand (P V forward; da,
dh, dctx, dx, dQ and every dW, dV, dK of the backward) on the bf16 matrix cores as three bf16 planes per operand and six products per
term (enc_gemm_bf16x3.hip), everything else the fp32 mode's launches.

The claim of the mode is fp32 accuracy, so the yardstick and the bound are the fp32 mode's own (tests/test_gpu_encoder_backward.py; its
_case, _compare and _group are used here, and _shape_case of tests/test_gpu_encoder_backward_shapes.py): the same model in float64 on the
CPU, per tensor bound(ref_err, max|grad|) = max(4 ref_err, 4 * 2^-23 max|grad|), ref_err the deviation of the same model's fp32 CPU
autograd from float64; the key bias is held to the query bias's scale.  Cases: 1 x (2, 5), 2 x (3, 37), 2 x (2, 130) of the first file,
row257 and heavy (trained-statistics weights, logits beyond +-30) of the second.  Its `tiles` case (5 599 rows at ffn 3072) is left
out: the large tiles and the long contraction are covered on the bare product by tests/test_gpu_gemm_bf16x3.py.

What else is checked: the mode is taken (GEMM_BF16X3_LAST moves in a step of the mode and not in a step of the fp32 mode, in this
process and in a fresh one); the forward's NT products are the fp32 mode's (qkv and the soft-max probabilities on the tape of a
one-layer forward have the fp32 mode's bits -- the tape keeps P, the in-place soft-max of the scores, not the scores; the context P V
may differ); forward_cls with and without a mix; dropout; a RankTrainer run resumed from a checkpoint.

Largest |kernel - float64| / bound per tensor group on an MI355X, the case where the ratio is largest (every comparison prints its
figures before it asserts):

    group                                  error       bound       ratio  case
    hidden                                 3.986e-05   6.389e-05   0.62   heavy 2 x (3, 96)
    tables                                 7.859e-03   2.098e-02   0.37   heavy 2 x (3, 96)
    emb LayerNorm                          1.644e-04   3.758e-04   0.44   heavy 2 x (3, 96)
    attention.self.query.weight            1.152e-02   2.213e-02   0.52   heavy 2 x (3, 96)
    attention.self.query.bias              1.485e-04   2.801e-04   0.53   heavy 2 x (3, 96)
    attention.self.key.weight              2.438e-03   4.258e-03   0.57   heavy 2 x (3, 96)
    attention.self.key.bias                1.788e-07   5.527e-07   0.32   1 x (2, 5)
    attention.self.value.weight            2.035e-03   6.223e-03   0.33   heavy 2 x (3, 96)
    attention.self.value.bias              2.582e-05   7.422e-05   0.35   heavy 2 x (3, 96)
    attention.output.dense.weight          1.279e-03   2.723e-03   0.47   heavy 2 x (3, 96)
    attention.output.dense.bias            1.141e-04   3.538e-04   0.32   heavy 2 x (3, 96)
    attention.output.LayerNorm.weight      9.594e-06   2.365e-05   0.41   2 x (3, 37)
    attention.output.LayerNorm.bias        1.527e-05   5.571e-05   0.27   heavy 2 x (3, 96)
    intermediate.dense.weight              2.967e-03   7.175e-03   0.41   heavy 2 x (3, 96)
    intermediate.dense.bias                3.555e-05   8.699e-05   0.41   heavy 2 x (3, 96)
    output.dense.weight                    7.842e-06   1.400e-05   0.56   1 x (2, 5)
    output.dense.bias                      1.448e-05   4.017e-05   0.36   row257 1 x (2, 257)
    output.LayerNorm.weight                2.418e-06   6.802e-06   0.36   1 x (2, 5)
    output.LayerNorm.bias                  7.264e-05   2.422e-04   0.30   heavy 2 x (3, 96)
    cls, learned mix                       8.270e-07   3.224e-06   0.26   2 x (3, 37)
    mix logits' gradient                   1.929e-06   3.819e-06   0.51   2 x (3, 37)
    cls, no mix                            9.694e-07   3.961e-06   0.24   2 x (3, 37)

The hidden state of `heavy` is close to the fp32 mode's own figure (3.509e-05 there: the forward differs in P V alone).  On its first run, with
all six terms of a product in one accumulator, `heavy` was outside at two tensors: layer 0's attention.output.LayerNorm.weight at
4.020e-04 of 2.981e-04 and output.LayerNorm.weight at 6.845e-04 of 4.387e-04 (the fp32 mode: 0.35 and 0.24 of the bound).  No bound was
moved: the matrix core cuts addends far below the running sum toward minus infinity, the same sign in every element of dx, and a gain
gradient sums dx over the token rows; the correction terms now have an accumulator of their own (enc_gemm_bf16x3.hip, NOTES.md), and
the two tensors sit at 0.30 and 0.26.  ctx = P V against the fp32 mode at 1 x (3, 37): 56 993 of 85 248 elements differ in bits, by at
most 1.788e-07 at max|ctx| 0.97.
"""
import copy
import functools
import os
import subprocess
import sys

import pytest
import torch

from test_gpu_encoder_backward import _bert, _case, _compare, _group, _mask  # noqa: F401  (_group: _compare's table)
from test_gpu_encoder_backward_shapes import _assert_heavy_statistics, _shape_case, _tag
from test_gpu_encoder_bf16 import TABLES, _batches, _trainer_bert
from test_gpu_gemm_bf16x3 import _last, product
from trainside_inputs import bound  # noqa: E402  (tests/golden: on the path once the lines above have run)
import bf16_matmul_ref as br  # noqa: E402
import readout_inputs as ri  # noqa: E402

pytestmark = pytest.mark.gpu
MODE = 'bf16x3'
CASES = [(1, 2, 5), (2, 3, 37), (2, 2, 130), 'row257', 'heavy']


def _ref(case):
    """-> m, tok, typ, mask, G, runs {float64 | float32: (hidden, {name: grad})}, tag"""
    if isinstance(case, str):
        return _shape_case(case)[:6] + (_tag(case),)
    n_layers, b, l = case
    return _case(n_layers, b, l) + (f'{n_layers} x ({b}, {l})',)


def _step(enc, tok, typ, mask, G):
    """one training forward + backward -> (hidden, {name: grad})"""
    enc.zero_grad(set_to_none=True)
    hidden = enc(tok, token_type_ids=typ, attention_mask=mask)
    (hidden * G.cuda()).sum().backward()
    return hidden.detach(), {n: p.grad.clone() for n, p in enc.bert.named_parameters()}


@functools.lru_cache(maxsize=None)
def _gpu_run(case, matmul):
    """a mode's step on a case, computed once and shared (never written to)"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G = _ref(case)[:5]
    return _step(HipBertTrainEncoder(copy.deepcopy(m), matmul=matmul).train(), tok, typ, mask, G)


@pytest.mark.parametrize('case', CASES, ids=str)
def test_parity_with_the_exact_float64_model_under_the_fp32_bound(case):
    if case == 'heavy':
        _assert_heavy_statistics()
    m, tok, typ, mask, G, runs, tag = _ref(case)
    before = _last()
    hidden, got = _gpu_run(case, MODE)
    assert hidden.is_cuda and hidden.shape == tok.shape + (768,)
    assert all(g is not None and torch.isfinite(g).all() for g in got.values())
    h64, h32 = runs[torch.float64][0], runs[torch.float32][0]
    tol = bound(float((h32.double() - h64).abs().max()), float(h64.abs().max()))
    err = float((hidden.double().cpu() - h64).abs().max())
    print(f'[{MODE} {tag}] hidden |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}  (GEMM_BF16X3_LAST {before} -> {_last()})')
    _compare(got, runs, f'{MODE} {tag}')
    assert err <= tol


def test_the_mode_is_taken():
    """GEMM_BF16X3_LAST after a pinned bare product reads TN 128 x 128, which no product of these shapes takes by the rule; a step of the
    fp32 mode leaves it there, a step of the mode moves it to a 64 x 64 instantiation.  Two steps of the mode: the same bits."""
    from aspire_amd import HipBertTrainEncoder, _lib
    m, tok, typ, mask, G = _ref((2, 3, 37))[:5]
    with _lib.pinned(GEMM_TILE='128'):
        _, inst = product(torch.ones(4, 4), torch.ones(4, 4), 2)
    assert inst == _last() == 6
    h32, g32 = _step(HipBertTrainEncoder(copy.deepcopy(m), matmul='fp32').train(), tok, typ, mask, G)
    assert _last() == 6
    hx3, gx3 = _step(HipBertTrainEncoder(copy.deepcopy(m), matmul=MODE).train(), tok, typ, mask, G)
    assert _last() in (5, 8), _last()
    diff = float((hx3 - h32).abs().max())
    print(f'max |hidden {MODE} - hidden fp32| at 2 x (3, 37): {diff:.3e}; gradients with other bits: '
          f'{sum(not torch.equal(gx3[n], g32[n]) for n in g32)} of {len(g32)}')
    assert any(not torch.equal(gx3[n], g32[n]) for n in g32)        # a switch that is silently ignored would give the fp32 mode's bits
    h2, g2 = _gpu_run((2, 3, 37), MODE)
    assert torch.equal(hx3, h2) and all(torch.equal(gx3[n], g2[n]) for n in g2)


CHILD = r'''
import copy, ctypes, sys
sys.path[:0] = [{root!r}, {tests!r}, {golden!r}]
import torch
from aspire_amd import HipBertTrainEncoder, _lib
import bf16_matmul_ref as br
def last():
    buf = ctypes.create_string_buffer(32)
    _lib.check(_lib.lib.aspire_debug_get(b'GEMM_BF16X3_LAST', buf, len(buf)))
    return int(buf.value)
m = br._bert(1)
tok, G = torch.randint(0, br.VOCAB, (2, 5)), torch.randn(2, 5, 768)
seen = [last()]
for mode in ('fp32', 'bf16x3'):
    enc = HipBertTrainEncoder(copy.deepcopy(m), matmul=mode).train()
    (enc(tok, token_type_ids=torch.zeros_like(tok), attention_mask=torch.ones_like(tok)) * G.cuda()).sum().backward()
    torch.cuda.synchronize()
    seen.append(last())
print('LAST', *seen)
'''


def test_a_fresh_process_in_fp32_mode_never_launches_the_kernel():
    """from a fresh process state: -1 before anything, still -1 after a step in the fp32 mode, an instantiation after a step in the mode"""
    tests = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(root=os.path.dirname(tests), tests=tests, golden=os.path.join(tests, 'golden'))
    out = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0
    line = next(ln for ln in out.stdout.splitlines() if ln.startswith('LAST'))
    first, after_fp32, after_mode = (int(x) for x in line.split()[1:])
    assert first == -1 and after_fp32 == -1 and after_mode in (5, 8), line


def _align(n):
    return (n + 255) // 256 * 256


def test_the_forwards_nt_products_are_the_fp32_modes():
    """one layer: the tape of the mode against the tape of the fp32 mode.  x and qkv (the QKV projection) and P (the soft-max, in place, of
    Q K^T: equal probabilities from the same fp32 kernel are equal scores) have the same bits; ctx = P V is the mode's own product and
    agrees to fp32 rounding; what follows ctx inherits its difference"""
    from aspire_amd import HipBertTrainEncoder
    import aspire_amd.torch_ops  # noqa: F401
    b, l = 3, 37
    m = _bert(1, seed=3)
    g = torch.Generator().manual_seed(8)
    tok, typ, mask = torch.randint(0, 50, (b, l), generator=g), torch.randint(0, 2, (b, l), generator=g), _mask(b, l)
    enc = HipBertTrainEncoder(copy.deepcopy(m))
    with torch.no_grad():
        emb = enc.bert.embeddings
        emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(typ.cuda())) + emb.position_embeddings.weight[:l]
        weights = [w.detach().clone() for w in enc.layer_weights()]
    tapes = {}
    for name, mode in (('fp32', 0), (MODE, 3)):
        hidden, tape = torch.ops.aspire.bert_layers_train_prec(emb_sum, mask.cuda(), weights, 12, 1e-12, 0.0, 0.0, 0, 0, mode)
        tapes[name] = tape.cpu()
    # the tape's layout (include/aspire_hip.h; encoder_bwd.hip): emb_sum, then per layer x | qkv | P | ctx | ..., every slot 256-byte aligned
    rows, lp = b * l, (l + 3) // 4 * 4
    sizes = [('x', rows * 768), ('qkv', rows * 2304), ('P', b * 12 * l * lp), ('ctx', rows * 768)]
    off, slots = _align(rows * 768 * 4), {}
    for name, n in sizes:
        slots[name] = (off, n)
        off += _align(n * 4)

    def slot(tape, name):
        o, n = slots[name]
        return tape[o:o + 4 * n].view(torch.float32)

    a, c = tapes['fp32'], tapes[MODE]
    assert a.shape == c.shape
    for name in ('x', 'qkv', 'P'):
        assert torch.equal(slot(a, name).view(torch.int32), slot(c, name).view(torch.int32)), name
    assert float(slot(a, 'P').sum()) > 1.0 and float(slot(a, 'qkv').abs().max()) > 0.1                    # (the slots hold what they are read as)
    ca, cc = slot(a, 'ctx'), slot(c, 'ctx')
    diff = float((ca - cc).abs().max())
    print(f'ctx = P V: {int((ca.view(torch.int32) != cc.view(torch.int32)).sum())} of {ca.numel()} elements differ in bits, largest '
          f'difference {diff:.3e} at max|ctx| {float(ca.abs().max()):.3e}')
    # either product is a sum of l terms p v with sum p = 1 in fp32: at most (l + 3) 2^-24 max|v| from the exact value (l roundings of the
    # sum, and the six-term product's dropped part 2^-23 |p| |v| with its own rounding), so the two are at most twice that apart
    vmax = float(slot(a, 'qkv').view(rows, 2304)[:, 1536:].abs().max())
    assert 0 < diff <= 2 * (l + 3) * 2.0 ** -24 * vmax


@functools.lru_cache(maxsize=None)
def _cls_refs(with_mix):
    """the CLS read-out of the 2 x (3, 37) case in float64 and in fp32 on the CPU (no emulation: the fp32 mode's yardstick)"""
    m, tok, typ, mask = _case(2, 3, 37)[:4]
    g = torch.Generator().manual_seed(7)
    G = torch.randn(3, 768, generator=g)
    logits = torch.randn(3, generator=g) if with_mix else None
    if with_mix:
        runs = {dt: br._run(m, dt, False, tok, typ, mask, G, logits) for dt in (torch.float64, torch.float32)}
    else:
        runs = {}
        for dt in (torch.float64, torch.float32):
            mm = copy.deepcopy(m).to(dt)
            y = mm(tok, token_type_ids=typ, attention_mask=mask).last_hidden_state[:, 0, :]
            (y * G.to(dt)).sum().backward()
            runs[dt] = (y.detach(), {n: p.grad for n, p in mm.named_parameters()}, None)
    return m, tok, typ, mask, G, logits, runs


@pytest.mark.parametrize('with_mix', [True, False], ids=['mix', 'no mix'])
def test_forward_cls(with_mix):
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G, logits, runs = _cls_refs(with_mix)
    tag = f'{MODE} cls 2 x (3, 37)' + (' mix' if with_mix else '')
    enc = HipBertTrainEncoder(copy.deepcopy(m), matmul=MODE).train()
    lg = logits.clone().cuda().requires_grad_(True) if with_mix else None
    cls = enc.forward_cls((tok, typ, mask), mix=torch.softmax(lg, 0)) if with_mix else enc.forward_cls((tok, typ, mask))
    assert cls.shape == (3, 768) and cls.requires_grad
    (cls * G.cuda()).sum().backward()
    (c, g, gl), (c32, g32, gl32) = runs[torch.float64], runs[torch.float32]
    tol = bound(float((c32.double() - c).abs().max()), float(c.abs().max()))
    err = float((cls.detach().double().cpu() - c).abs().max())
    print(f'[{tag}] cls |kernel - float64| {err:.3e}  bound {tol:.3e}  ratio {err / tol:.2f}')
    if with_mix:
        tol_l = bound(float((gl32.double() - gl).abs().max()), float(gl.abs().max()))
        err_l = float((lg.grad.double().cpu() - gl).abs().max())
        print(f'[{tag}] mix logits\' gradient |kernel - float64| {err_l:.3e}  bound {tol_l:.3e}  ratio {err_l / tol_l:.2f}')
    _compare({n: p.grad for n, p in enc.bert.named_parameters()}, {torch.float64: (c, g), torch.float32: (c32, g32)}, tag)
    assert err <= tol
    if with_mix:
        assert err_l <= tol_l
    else:       # the CLS rows of the mode's last hidden state
        assert torch.equal(cls.detach(), _gpu_run((2, 3, 37), MODE)[0][:, 0, :])


def test_dropout_in_the_mode():
    """the same (seed, step) gives the same bits twice; p = 0 gives the no-dropout bits of the mode"""
    from aspire_amd import HipBertTrainEncoder
    m, tok, typ, mask, G = _ref((2, 3, 37))[:5]

    def run(p, state):
        mm = copy.deepcopy(m)
        mm.config.hidden_dropout_prob = mm.config.attention_probs_dropout_prob = p
        enc = HipBertTrainEncoder(mm, dropout=True, seed=77, matmul=MODE).train()
        enc.set_dropout_state(*state)
        out = _step(enc, tok, typ, mask, G)
        assert enc.dropout_state() == (state[0], state[1] + 1)
        return out

    h1, g1 = run(0.1, (77, 5))
    h2, g2 = run(0.1, (77, 5))
    assert torch.equal(h1, h2) and all(torch.equal(g1[n], g2[n]) for n in g1)
    h3, _ = run(0.1, (77, 6))
    assert not torch.equal(h1, h3)
    h0, g0 = run(0.0, (77, 5))
    hn, gn = _gpu_run((2, 3, 37), MODE)
    assert not torch.equal(h1, h0)
    assert torch.equal(h0, hn) and all(torch.equal(g0[n], gn[n]) for n in g0)


def test_trainer_resumes_on_the_straight_runs_bits(tmp_path):
    """RankTrainer in the mode with dropout, the tables frozen (their scatter gradient is torch's): four iterations straight, and two + a
    checkpoint + two, end on the same bits; the checkpoint names its mode, and an fp32 and a bf16 encoder refuse it by name"""
    from aspire_amd import HipBertTrainEncoder, RankTrainer
    batches = _batches(str(tmp_path))
    hparams = ri.hparams('l2wasserstein', 0.0)
    train_hparams = dict(es_check_every=1000, train_size=6, dev_size=3, batch_size=3, num_epochs=2, update_rule='adam', learning_rate=1e-3,
                         lr_decay_method='exponential', decay_lr_by=0.7, decay_lr_every=1)

    def make(seed, tag, matmul=MODE):
        model = _trainer_bert(seed)
        for n, p in model.named_parameters():
            if n in TABLES:
                p.requires_grad_(False)
        enc = HipBertTrainEncoder(model, dropout=True, seed=0x9E3779B97F4A7C15, matmul=matmul)
        return RankTrainer(enc, hparams, train_hparams, str(tmp_path / tag), lambda epoch: batches)

    straight = make(5, 'straight')
    straight.train(max_iterations=4)
    first = make(5, 'first')
    first.train(max_iterations=2)
    first.save_checkpoint(tmp_path / 'ck.pt')
    assert torch.load(tmp_path / 'ck.pt', weights_only=True)['matmul'] == MODE
    second = make(99, 'second')
    second.load_checkpoint(tmp_path / 'ck.pt')
    second.train(max_iterations=2)
    assert second.iteration == straight.iteration == 4
    trained = 0
    for (n, a), (_, b) in zip(second.encoder.bert.named_parameters(), straight.encoder.bert.named_parameters()):
        assert torch.isfinite(a).all() and torch.equal(a, b), n
        sa, sb = second.optimizer.state.get(a, {}), straight.optimizer.state.get(b, {})
        assert set(sa) == set(sb), n
        for key in sa:
            assert torch.equal(sa[key], sb[key]), (n, key)
        trained += bool(sa)
    assert trained >= 16
    for other in ('fp32', 'bf16'):
        with pytest.raises(ValueError, match=f"'{MODE}'.*'{other}'"):
            make(5, 'other_' + other, matmul=other).load_checkpoint(tmp_path / 'ck.pt')
