/* A plain-C caller of the orthogonal read: the reference's zarrita fixture
 * (tests/golden/zarrita, i2 4x5x6 in 2x3x4 gzip chunks) opened through
 * zcg_array_meta_from_json, and the selection rows {3, 0} x columns {4, 1, 6}
 * x planes {5, 2, 2} read with ONE zcg_store_read_ortho call: unsorted lists,
 * an index twice, and the first index past the grid along dimension 1, whose
 * elements are filled.  zcg_ortho_chunks tells the chunks the selection
 * touches.  The 18 values, C order over the positions, are written to <out
 * file>; the test compares them with values it computes itself.
 * Usage: ortho_c <store root> <out file> [device].  Prints "ortho_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_VALUES 18

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: ortho_c <store root> <out file> [device]\n"); return 2; }
    const char* root = argv[1];
    const int device = argc > 3 ? atoi(argv[3]) : 0;
    char mpath[4096];
    snprintf(mpath, sizeof mpath, "%s/meta/root/seq/i2.array.json", root);
    FILE* f = fopen(mpath, "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", mpath); return 2; }
    static char json[65536];
    const size_t jlen = fread(json, 1, sizeof json, f);
    fclose(f);
    zcg_array_meta m;
    char err[256];
    int st = zcg_array_meta_from_json(json, jlen, &m, err, sizeof err);
    if (st != ZCG_OK) { fprintf(stderr, "array metadata: %d %s\n", st, err); return 1; }
    if (m.ndim != 3 || m.array.dtype.elem_size != 2) { fprintf(stderr, "unexpected metadata\n"); return 1; }

    const uint64_t rows[2] = {3, 0}, cols[3] = {4, 1, 6}, planes[3] = {5, 2, 2};
    const uint64_t* lists[ZCG_MAX_DIMS] = {rows, cols, planes};
    const uint64_t count[ZCG_MAX_DIMS] = {2, 3, 3};
    int16_t vals[N_VALUES];
    memset(vals, 0xA5, sizeof vals);

    zcg_region r;
    memset(&r, 0, sizeof r);
    r.ndim = m.ndim;
    for (uint32_t d = 0; d < m.ndim; d++) { r.array_shape[d] = m.shape[d]; r.chunk_shape[d] = m.chunk_shape[d]; }
    uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS];
    uint8_t touched[3 * 8];
    memset(touched, 0, sizeof touched);
    const uint64_t chunks = zcg_ortho_chunks(&r, lists, count, lo, n, NULL);
    if (n[0] + n[1] + n[2] > sizeof touched) { fprintf(stderr, "unexpected grid range\n"); return 1; }
    if (zcg_ortho_chunks(&r, lists, count, lo, n, touched) != chunks) { fprintf(stderr, "chunk counts differ\n"); return 1; }

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_read_ortho(ctx, &m, root, "/seq/i2", lists, count, vals, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_ortho: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f || fwrite(vals, 1, sizeof vals, f) != sizeof vals) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("ortho_c: ok (%d elements, %llu touched chunks, scratch %llu bytes)\n", N_VALUES,
           (unsigned long long)chunks, (unsigned long long)zcg_ortho_scratch_bytes(3, count));
    return 0;
}
