"""CPU: the C-ABI library loads and exports every symbol include/aspire_hip.h declares (no compute
calls -- there is no GPU here), argument validation that needs no device, and the host-side prep."""
import json
import os
import re

import pytest
import torch


def _header_functions(root):
    src = open(os.path.join(root, 'include', 'aspire_hip.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(aspire_[a-z0-9_]+)\s*\(', src)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from aspire_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = _header_functions(root)
    assert len(declared) >= 9
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), f'{name} declared in aspire_hip.h but not exported'
        assert name in _lib.SIGNATURES, f'{name} has no ctypes signature in aspire_amd/_lib.py'
    assert sorted(_lib.SIGNATURES) == declared
    assert _lib.lib.aspire_abi_version() == 6
    assert _lib.lib.aspire_max_sents() == 128


def test_no_product_module_imports_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, 'aspire_amd')):
        for f in files:
            if f.endswith(('.py', '.hip', '.h', '.cpp')):
                text = open(os.path.join(dirpath, f)).read()
                assert 'oracle' not in text.replace('the oracle', '').replace("oracle's", ''), f


def test_argument_validation_without_gpu():
    import ctypes
    from aspire_amd import _lib
    q = _lib.RepSet(0, 0, 0, 2, 4, 4)
    c = _lib.RepSet(0, 0, 0, 3, 4, 4)
    # pair_distances.py:46 assert (qef_batch_size == cef_batch_size)
    rc = _lib.lib.aspire_l2max_scores_f32(ctypes.byref(q), ctypes.byref(c), 768, _lib.PAIR_PAIRED, 0, 1, 0, None)
    assert rc == _lib.ASPIRE_ERR_INVALID_ARG
    with pytest.raises(AssertionError):
        _lib.check(rc)
    rc = _lib.lib.aspire_l2max_scores_f32(ctypes.byref(q), ctypes.byref(c), 512, _lib.PAIR_CROSS, 0, 1, 0, None)
    assert rc == _lib.ASPIRE_ERR_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _lib.check(rc)
    assert b'768' in _lib.lib.aspire_last_error()


def test_diagnostic_switches_without_gpu():
    """aspire_debug_set accepts the documented keys / values, rejects others, and restores defaults on NULL."""
    from aspire_amd import _lib
    assert _lib.lib.aspire_debug_set(b'SINKHORN', b'block') == _lib.ASPIRE_OK
    assert _lib.lib.aspire_debug_set(b'SINKHORN', None) == _lib.ASPIRE_OK
    assert _lib.lib.aspire_debug_set(b'SINKHORN', b'packed') == _lib.ASPIRE_ERR_INVALID_ARG     # a form that is no longer built
    assert _lib.lib.aspire_debug_set(b'NO_SUCH_SWITCH', b'1') == _lib.ASPIRE_ERR_INVALID_ARG
    with _lib.pinned(COST_PATH='valu', OT_FORM='tile'):
        pass
    with pytest.raises(AssertionError):
        with _lib.pinned(COST_PATH='bogus'):
            pass
    # a pin restores what was set BEFORE it (an enclosing pin, an ASPIRE_HIP_* setting), not the library default
    import ctypes
    buf = ctypes.create_string_buffer(64)

    def current(key):
        assert _lib.lib.aspire_debug_get(key, buf, len(buf)) == _lib.ASPIRE_OK
        return buf.value

    with _lib.pinned(OT_FORM='small', FUSED_WAVES=1024):
        with _lib.pinned(OT_FORM='fused'):
            assert current(b'OT_FORM') == b'fused'
        assert current(b'OT_FORM') == b'small' and current(b'FUSED_WAVES') == b'1024'
    assert current(b'OT_FORM') == b'' and current(b'FUSED_WAVES') == b''
    with _lib.pinned(TILE_WAVES=12):
        assert current(b'TILE_WAVES') == b'12'
    assert current(b'TILE_WAVES') == b''
    assert _lib.lib.aspire_debug_get(b'NO_SUCH_SWITCH', buf, len(buf)) == _lib.ASPIRE_ERR_INVALID_ARG


def test_no_getenv_on_the_launch_path():
    """The environment is read once, in lib.hip's tuning_from_env; no other product source calls getenv."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, 'aspire_amd', 'csrc')
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.h')) and f != 'lib.hip':
            assert 'getenv' not in open(os.path.join(csrc, f)).read(), f


def test_batch_entry_validation_without_gpu():
    import ctypes
    from aspire_amd import _lib
    q = _lib.RepSet(0, 0, 0, 2, 0, 8)
    c = _lib.RepSet(0, 0, 0, 30, 0, 8)
    prm = _lib.OtParams(0.05, 0.9, 1.0, 0)
    need = _lib.lib.aspire_ot_rank_batch_workspace_bytes(ctypes.byref(q), ctypes.byref(c), 20, 10)
    assert need >= 30 * 516 and need % 16 == 0
    # null job_off / workspace too small / padded rep sets are argument errors, not crashes
    args = lambda job_off, ws, nbytes: _lib.lib.aspire_ot_rank_batch_f32(
        ctypes.byref(q), ctypes.byref(c), 768, job_off, 20, ctypes.byref(prm), _lib.OT_SIMILARITY, 16, 10, None, 16, 16, None, ws, nbytes, None)
    assert args(None, 16, need) == _lib.ASPIRE_ERR_INVALID_ARG
    assert args(16, 16, need - 16) == _lib.ASPIRE_ERR_INVALID_ARG
    qp = _lib.RepSet(0, 0, 0, 2, 8, 8)
    assert _lib.lib.aspire_ot_rank_batch_f32(ctypes.byref(qp), ctypes.byref(c), 768, 16, 20, ctypes.byref(prm), _lib.OT_SIMILARITY,
                                             16, 10, None, 16, 16, None, 16, need, None) == _lib.ASPIRE_ERR_INVALID_ARG
    # the OT workspace is a multiple of 16 bytes (the 64-bit rank scratch sits right behind it)
    for qn, cn in ((1, 4097), (3, 4099), (1, 7)):
        q1, c1 = _lib.RepSet(0, 0, 0, qn, 0, 8), _lib.RepSet(0, 0, 0, cn, 0, 8)
        assert _lib.lib.aspire_ot_workspace_bytes(ctypes.byref(q1), ctypes.byref(c1), _lib.PAIR_CROSS) % 16 == 0
    # full sorts beyond one chunk have a workspace now (they were refused in round 1)
    assert _lib.lib.aspire_topk_workspace_bytes(1, 50000, 50000) == 2 * 13 * 4096 * 8


def _top_level_args(text):
    depth, n, cur = 0, 0, ''
    for ch in text:
        if ch in '([{':
            depth += 1
        elif ch in ')]}':
            depth -= 1
        if ch == ',' and depth == 0:
            n += 1 if cur.strip() else 0
            cur = ''
        else:
            cur += ch
    return n + (1 if cur.strip() else 0)


def test_integration_md_stub_passes_every_argument():
    """The ctypes stub shown in INTEGRATION.md must pass exactly the parameters include/aspire_hip.h declares (round 1's
    stub dropped workspace / workspace_bytes: the stream landed in the workspace slot)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    for fn in ('aspire_ot_sinkhorn_f32', 'aspire_ot_workspace_bytes'):
        decl = re.search(fn + r'\s*\((.*?)\)\s*;', hdr, flags=re.S).group(1)
        start = doc.index('lib.' + fn + '(') + len('lib.' + fn + '(')
        depth, end = 1, start
        while depth:
            depth += {'(': 1, ')': -1}.get(doc[end], 0)
            end += 1
        call = doc[start:end - 1]
        assert _top_level_args(call) == _top_level_args(decl), (fn, _top_level_args(call), _top_level_args(decl))


def _header_struct_fields(hdr, name):
    body = re.search(r'typedef struct \{((?:(?!typedef struct).)*?)\}\s*' + name + r'\s*;', hdr, flags=re.S).group(1)
    names = []
    for decl in body.split(';'):
        if decl.strip():      # "const float *w_qkv, *b_qkv" declares two
            parts = decl.strip().split(',')
            names += [re.sub(r'\[.*\]', '', p.strip().split()[-1].lstrip('*')) for p in parts]
    return names


def test_struct_fields_match_the_header():
    """every ctypes.Structure of aspire_amd/_lib.py AND of the stub in INTEGRATION.md lists the header's fields, in order
    (INTEGRATION.md's OtParams once stopped at cdist_mode: it only worked because ctypes zero-fills the tail)"""
    from aspire_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'aspire_hip.h')).read(), flags=re.S)
    doc = open(os.path.join(root, 'INTEGRATION.md')).read()
    for cname, cls in (('aspire_repset', _lib.RepSet), ('aspire_ot_params', _lib.OtParams), ('aspire_rep_planes', _lib.RepPlanes),
                       ('aspire_bert_layer', _lib.BertLayer), ('aspire_bert_weights', _lib.BertWeights)):
        assert [f[0] for f in cls._fields_] == _header_struct_fields(hdr, cname), cname
    for cname, pyname in (('aspire_repset', 'RepSet'), ('aspire_ot_params', 'OtParams')):
        block = re.search(r'class ' + pyname + r'\(ctypes\.Structure\):.*?_fields_ = \[(.*?)\]\s*(?:#.*)?\n(?:class|\n|def)', doc, flags=re.S).group(1)
        assert re.findall(r"\('(\w+)'", block) == _header_struct_fields(hdr, cname), pyname


def test_compute_requires_gpu():
    from aspire_amd import ops
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.DeviceRepSet.from_list([torch.zeros(2, 768)])


def _tokenizer(vocab, tmp_path):
    from transformers import BertTokenizer
    p = tmp_path / 'vocab.txt'
    p.write_text('\n'.join(vocab) + '\n')
    return BertTokenizer(str(p), do_lower_case=True)


def test_prepare_abstracts_matches_reference(golden_dir, tmp_path):
    """A0 against the reference's own prepare_abstracts output (tests/golden/prep.json), including the
    500-word-piece cap hit mid sentence, hit exactly (sentence dropped), and a one-piece remainder."""
    from aspire_amd import prepare_abstracts
    z = json.load(open(os.path.join(golden_dir, 'prep.json')))
    from transformers import BertTokenizerFast
    slow = _tokenizer(z['vocab'], tmp_path)
    # a fast (Rust) tokenizer goes through ONE batched call per prepare_abstracts instead of tokenize() per sentence: the same outputs
    for tok in (slow, BertTokenizerFast(str(tmp_path / 'vocab.txt'), do_lower_case=True)):
        for case in z['cases']:
            batch = [z['docs'][i] for i in case['doc_ids']]
            bert_batch, abs_lens, sent_token_idxs = prepare_abstracts(batch, tok)
            assert bert_batch['tokid_tt'].tolist() == case['tokid_tt']
            assert bert_batch['seg_tt'].tolist() == case['seg_tt']
            assert bert_batch['attnmask_tt'].tolist() == case['attnmask_tt']
            assert bert_batch['seq_lens'] == case['seq_lens']
            assert abs_lens == case['abs_lens']
            assert sent_token_idxs == case['sent_token_idxs']
            assert bert_batch['tokid_tt'].dtype == torch.int64
    from aspire_amd.batch_prep import prepare_bert_sentences
    sents = [[d['TITLE'] + ' [SEP] '] + list(d['ABSTRACT']) for d in z['docs'][:4]]
    assert prepare_bert_sentences(sents, slow)[1] == prepare_bert_sentences(sents, BertTokenizerFast(str(tmp_path / 'vocab.txt'), do_lower_case=True))[1]


def test_spans_to_csr():
    from aspire_amd.batch_prep import spans_to_csr
    tok, off = spans_to_csr([[[1, 2], [3]], [[5, 6, 7]]], 3)
    assert tok.tolist() == [1, 2, 3, 5, 6, 7]
    assert off.tolist() == [0, 2, 3, 3, 6, 6, 6]
    assert tok.dtype == torch.int32 and off.dtype == torch.int32


def test_header_is_plain_c_and_links(tmp_path):
    """include/aspire_hip.h is what a C caller (or a cgo / JNI stub) binds: it must compile as C99 with nothing but
    the standard headers, and a program that references every entry point must link against the library.  The
    program only takes addresses and calls the two host-only queries (no GPU here)."""
    import subprocess
    from aspire_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = _header_functions(root)
    src = tmp_path / 'abi_check.c'
    src.write_text('#include <stdio.h>\n#include "aspire_hip.h"\n'
                   'typedef void (*fn_t)(void);\n'
                   'int main(void) {\n  fn_t fns[] = {' + ', '.join(f'(fn_t){n}' for n in names) + '};\n'
                   '  aspire_repset r; aspire_ot_params p; (void)r; (void)p;\n'
                   '  if (aspire_abi_version() != ASPIRE_ABI_VERSION || aspire_max_sents() != 128) return 1;\n'
                   '  if (aspire_ot_workspace_bytes(0, 0, ASPIRE_PAIR_CROSS) != 0) return 2;\n'
                   '  if (aspire_topk_desc_f32(0, 1, 1, 0, 0, 0, 0, 0, 0, 0) != ASPIRE_ERR_INVALID_ARG) return 3;\n'
                   '  printf("%d %s\\n", (int)(sizeof(fns) / sizeof(fns[0])), aspire_last_error());\n  return 0;\n}\n')
    exe = tmp_path / 'abi_check'
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call(['gcc', '-std=c99', '-Wall', '-Werror', '-pedantic', f'-I{root}/include', str(src), '-o', str(exe),
                           f'-L{libdir}', '-laspire_hip', f'-Wl,-rpath,{libdir}', '-Wl,-rpath,/opt/rocm/lib'])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stdout.split()[0] == str(len(names)) and len(out.stdout.split()) > 1      # count + the error text


def test_kernel_register_budgets():
    """Co-residency budgets, read from the built code objects' metadata (tools/kernel_resources.py).  A SIMD has 512
    registers per lane: the headline workload overlaps many queries' launches, which only works while the small-pool
    cost kernel's resident waves leave room for the Sinkhorn / top-k waves of other queries (with a 256-register cost
    kernel bench.py fell from ~110 to ~70 M alignments/s, every kernel's own time unchanged)."""
    import sys
    from aspire_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, 'tools'))
    try:
        from kernel_resources import kernel_resources
    finally:
        sys.path.pop(0)
    res = kernel_resources(_lib.LIB_PATH)
    assert len(res) > 40

    def one(pattern):
        hits = [v for k, v in res.items() if re.search(pattern, k)]
        assert len(hits) == 1, (pattern, len(hits))
        return hits[0]

    cost = one(r'17pair_cost1_kernelE')          # two register sets (every launch of up to a few thousand pairs)
    sink = one(r'sinkhorn_kernelILi1E')
    topk = one(r'topk_select_kernelILi4E')
    assert cost['vgpr'] <= 200 and cost['scratch'] == 0
    sub = one(r'pair_cost1_sub_kernel')             # sub-tile form (long documents, small pools): capped, see cost_valu.hip
    assert sub['vgpr'] <= 216 and sub['scratch'] == 0
    assert sink['vgpr'] <= 56 and sink['scratch'] == 0
    assert topk['vgpr'] <= 56 and topk['scratch'] == 0
    # two (three) cost waves + two Sinkhorn / top-k waves per SIMD fit together
    granule = lambda v: (v + 7) // 8 * 8
    assert 2 * granule(cost['vgpr']) + 2 * granule(sink['vgpr']) <= 512
    # no scoring / ranking / encoder kernel spills (round 1's 32- / 64-column Gram forms did: 80 / 144 bytes)
    for name, r in res.items():
        assert r['scratch'] == 0, name
    # the fused otAspire kernel (table-driven and with in-wave tables): two 4-wave workgroups per CU (256 registers,
    # 43.5 KB of LDS each)
    fused = [v for k, v in res.items() if re.search(r'pair_fused_kernelILb1ELb1E', k)]
    assert len(fused) == 4          # table-driven, in-wave tables (batches), in-wave query box (one query x a pool), CHUNK items
    for r in fused:
        assert r['vgpr'] + r['agpr'] <= 256
    for bn in (32, 64):
        for r in (v for k, v in res.items() if re.search(rf'pair_gram_kernelILi{bn}E', k)):
            assert r['vgpr'] <= 256 and r['scratch'] == 0
    # the one-wave-per-pair forward kernels: two waves per SIMD.  jointsm_pair_kernel's 164 depends on the form of pair_fwd.h's
    # tile_row_valid / tile_row (a struct or a bool parameter there gave 176: NOTES.md, "The pair forward kernels' shared frame")
    jsm = one(r'jointsm_pair_kernel')
    assert jsm['vgpr'] <= 164 and jsm['vgpr'] + jsm['agpr'] <= 256
    for r in (v for k, v in res.items() if re.search(r'l2agg_pair_kernel', k)):
        assert r['vgpr'] <= 180 and r['vgpr'] + r['agpr'] <= 256
