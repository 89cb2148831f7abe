"""SHA-256 of forward_hidden per attention form, of forward_cls per GEMM / attention form and of the training operators' outputs, for
comparing two builds of the library bit for bit (NOTES.md, "attention on any mask" and "The encoder's shared host layer").

    python tools/attn_bits.py [parent_lib.so]

Without an argument: prints one line per (shape, form) for the library in the tree (or ASPIRE_HIP_LIB).  With a second library: runs
itself in a fresh child process per library (the second one through ASPIRE_HIP_LIB) and reports which lines differ.  Shapes: those of
tests/test_gpu_attn_planes.py::test_plane_attention_has_the_bits_of_the_round5_kernel (prefix masks, ragged) and the MPNet batch of
tests/test_gpu_sbert.py (6 x 200).  `cls-` lines: forward_cls (cls_out and layer_cls in one digest) of a 2-layer model without and with a
layer mix; `train-` lines: torch.ops.aspire.bert_layers_train / bert_layers_backward called directly (hidden; grad_emb_sum and every
parameter gradient in order -- not the tape, whose gaps are unwritten) for 0 and 2 layers."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {'p': dict(GEMM='planes'), 'p64': dict(GEMM='planes', ATTN='p64'), 'planes-f16x2': dict(GEMM='planes', ATTN='f16x2'),
         'f16x2': dict(GEMM='bf16x3'), 'f32': dict(GEMM='bf16x3', ATTN='f32'), 'gemm': dict(ATTN='gemm')}
SHAPES = [(2, 8, 128), (1, 64, 256), (2, 4, 512), (1, 16, 64), (2, 3, 400), (1, 52, 128)]
CLS_FORMS = {'default': {}, 'attn-gemm': dict(ATTN='gemm'), 'gemm-f32': dict(GEMM='f32'), 'planes': dict(GEMM='planes')}
CLS_SHAPES = [(3, 40), (5, 130)]
TRAIN_CASES = [(n, b, l) for n in (0, 2) for b, l in ((2, 40), (3, 130))]


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def child():
    sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
    import torch  # noqa: F401
    from aspire_amd._lib import pinned
    from aspire_amd.encoder import HipBertEncoder
    from test_gpu_encoder import _batch, _bert
    from test_gpu_sbert import _inputs, _model

    def digest(enc, ids, seg, mask, tag, forms):
        for form in forms:
            with pinned(**FORMS[form]):
                out = enc.forward_hidden(ids, seg, mask).cpu()
            assert enc.status() == 0 and bool(torch.isfinite(out).all()), (tag, form)
            print(f'BITS {tag} {form} {hashlib.sha256(out.numpy().tobytes()).hexdigest()}', flush=True)

    for n_layers, b, l in SHAPES:
        tok, seg, mask, _ = _batch(b, l, 3000, seed=900 + l)
        digest(HipBertEncoder(_bert(n_layers, seed=40 + l)), tok, seg, mask, f'bert-{n_layers}x{b}x{l}', FORMS)
    ids, mask = _inputs('mpnet')
    digest(HipBertEncoder(_model('mpnet')), ids, None, mask, 'mpnet-2x6x200', [f for f in FORMS if f != 'p64'])

    enc = HipBertEncoder(_bert(2, seed=77))
    for b, l in CLS_SHAPES:
        tok, seg, mask, _ = _batch(b, l, 3000, seed=700 + l)
        for mix in (None, torch.softmax(torch.tensor([0.3, -0.2, 0.9]), 0).tolist()):
            for form, pins in CLS_FORMS.items():
                with pinned(**pins):
                    out, layers = enc.forward_cls(tok, seg, mask, layer_mix=mix, want_layers=True)
                assert enc.status() == 0 and bool(torch.isfinite(out).all()) and bool(torch.isfinite(layers).all()), (b, l, form)
                print(f'BITS cls-2x{b}x{l}{"-mix" if mix else ""} {form} {sha(out, layers)}', flush=True)

    import aspire_amd.torch_ops  # noqa: F401  (registers the operators)
    from aspire_amd import HipBertTrainEncoder
    from test_gpu_encoder_backward import VOCAB, _bert as _train_bert
    for n_layers, b, l in TRAIN_CASES:
        tenc = HipBertTrainEncoder(_train_bert(n_layers, seed=3 + n_layers))
        tok, seg, mask, _ = _batch(b, l, VOCAB, seed=800 + l)
        with torch.no_grad():
            emb = tenc.bert.embeddings
            emb_sum = (emb.word_embeddings(tok.cuda()) + emb.token_type_embeddings(seg.cuda())) + emb.position_embeddings.weight[:l]
            weights = [w.detach().clone() for w in tenc.layer_weights()]
        grad_hidden = torch.randn(b, l, 768, generator=torch.Generator().manual_seed(900 + l)).cuda()
        hidden, tape = torch.ops.aspire.bert_layers_train(emb_sum, mask.cuda(), weights, 12, 1e-12)
        grad_emb, grads = torch.ops.aspire.bert_layers_backward(grad_hidden, tape, mask.cuda(), weights, 12, 1e-12)
        assert all(bool(torch.isfinite(t).all()) for t in (hidden, grad_emb, *grads)) and len(grads) == len(weights), (n_layers, b, l)
        print(f'BITS train-{n_layers}x{b}x{l} hidden {sha(hidden)}', flush=True)
        print(f'BITS train-{n_layers}x{b}x{l} grads {sha(grad_emb, *grads)}', flush=True)


def main():
    if len(sys.argv) < 2:
        return child()
    runs = []
    for lib in (None, sys.argv[1]):
        env = dict(os.environ)
        if lib:
            env['ASPIRE_HIP_LIB'] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            sys.exit(f'{lib or "tree"}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        runs.append({tuple(x.split()[1:3]): x.split()[3] for x in r.stdout.splitlines() if x.startswith('BITS ')})
    tree, other = runs
    assert tree.keys() == other.keys() and tree
    diff = [k for k in tree if tree[k] != other[k]]
    for k in tree:
        print(f'{k[0]:18s} {k[1]:13s} {tree[k][:16]}  {"same bits" if tree[k] == other[k] else "DIFFERENT: " + other[k][:16]}')
    print(f'{len(tree)} digests, {len(diff)} differ')
    sys.exit(1 if diff else 0)


main()
