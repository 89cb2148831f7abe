"""SHA-256 of forward_hidden per attention form, for comparing two builds of the library bit for bit (NOTES.md, "attention on any mask").

    python tools/attn_bits.py [parent_lib.so]

Without an argument: prints one line per (shape, form) for the library in the tree (or ASPIRE_HIP_LIB).  With a second library: runs
itself in a fresh child process per library (the second one through ASPIRE_HIP_LIB) and reports which lines differ.  Shapes: those of
tests/test_gpu_attn_planes.py::test_plane_attention_has_the_bits_of_the_round5_kernel (prefix masks, ragged) and the MPNet batch of
tests/test_gpu_sbert.py (6 x 200)."""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {'p': dict(GEMM='planes'), 'p64': dict(GEMM='planes', ATTN='p64'), 'planes-f16x2': dict(GEMM='planes', ATTN='f16x2'),
         'f16x2': dict(GEMM='bf16x3'), 'f32': dict(GEMM='bf16x3', ATTN='f32'), 'gemm': dict(ATTN='gemm')}
SHAPES = [(2, 8, 128), (1, 64, 256), (2, 4, 512), (1, 16, 64), (2, 3, 400), (1, 52, 128)]


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
