/* A plain-C caller of the point read: the reference's zarrita fixture
 * (tests/golden/zarrita, i2 4x5x6 in 2x3x4 gzip chunks) opened through
 * zcg_array_meta_from_json, and seven elements read by coordinate with ONE
 * zcg_store_read_points call: both corners of the array, interior points of
 * four different chunks, one coordinate twice, and a point beyond the array
 * (the first index past the grid along dimension 1), which is filled.
 * zcg_points_grid tells the grid range the points need and zcg_points_last
 * which of them a write would keep.  The seven values are written to <out
 * file>; the test compares them with values it computes itself.
 * Usage: points_c <store root> <out file> [device].  Prints "points_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_POINTS 7

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: points_c <store root> <out file> [device]\n"); return 2; }
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

    const uint64_t coords[N_POINTS * 3] = {0, 0, 0, 3, 4, 5, 1, 2, 3, 2, 3, 4, 1, 2, 3, 0, 6, 1, 3, 0, 2};
    int16_t vals[N_POINTS];
    memset(vals, 0xA5, sizeof vals);

    zcg_region r;
    memset(&r, 0, sizeof r);
    r.ndim = m.ndim;
    for (uint32_t d = 0; d < m.ndim; d++) { r.array_shape[d] = m.shape[d]; r.chunk_shape[d] = m.chunk_shape[d]; }
    uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS];
    const uint64_t range = zcg_points_grid(&r, coords, N_POINTS, lo, n);
    uint8_t keep[N_POINTS];
    const uint64_t kept = zcg_points_last(coords, N_POINTS, 3, keep);

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_read_points(ctx, &m, root, "/seq/i2", coords, N_POINTS, vals, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_points: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f || fwrite(vals, 1, sizeof vals, f) != sizeof vals) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("points_c: ok (%d points, grid range %llu chunks, %llu kept, keep[2] = %d)\n", N_POINTS,
           (unsigned long long)range, (unsigned long long)kept, (int)keep[2]);
    return 0;
}
