// The encoder's five buffer-size queries over a grid of geometries and shapes, one line each: the table two builds of the library must
// agree on when only the host code that carves those buffers changed (NOTES.md, "The encoder's shared host layer").  Host only: the
// queries read the struct's geometry, no pointer, and make no GPU call.
//
//   c++ -std=c++17 tools/enc_sizes.cpp -Laspire_amd/lib -laspire_hip -o enc_sizes
//   LD_LIBRARY_PATH=<dir of build A> ./enc_sizes > a.txt; LD_LIBRARY_PATH=<dir of build B> ./enc_sizes > b.txt; cmp a.txt b.txt
//
// To have a sanitizer watch the carving itself, compile the two host files in (their definitions then take the place of the
// library's, which still supplies the launchers they name but never call here):
//   hipcc --offload-arch=gfx950 -std=c++17 -g -Xarch_host -fsanitize=address,undefined tools/enc_sizes.cpp aspire_amd/csrc/encoder.hip
//         aspire_amd/csrc/encoder_bwd.hip -Laspire_amd/lib -laspire_hip -o enc_sizes_san         (one command line)
#include <stdio.h>

#include "../include/aspire_hip.h"

int main() {
    const int layers[] = {0, 2, 12}, ffns[] = {3072, 1024};
    const long long shapes[][2] = {{1, 1}, {2, 40}, {3, 130}, {5, 511}, {64, 256}};
    printf("n_layers ffn_dim B L workspace cls_workspace tape train_workspace planes\n");
    for (int n : layers)
        for (int ffn : ffns)
            for (const auto& s : shapes) {
                aspire_bert_weights w = {};
                w.n_layers = n;
                w.n_heads = 12;
                w.hidden = 768;
                w.ffn_dim = ffn;
                w.vocab = 30522;
                w.max_pos = 512;
                w.n_types = 2;
                w.ln_eps = 1e-12f;
                printf("%d %d %lld %lld %zu %zu %zu %zu %zu\n", n, ffn, s[0], s[1], aspire_bert_workspace_bytes(&w, s[0], s[1]),
                       aspire_bert_cls_workspace_bytes(&w, s[0], s[1]), aspire_bert_tape_bytes(&w, s[0], s[1]),
                       aspire_bert_train_workspace_bytes(&w, s[0], s[1]), aspire_bert_planes_bytes(&w));
            }
    return 0;
}
