/* A plain-C caller of the batched box read for boxes of differing shapes: the
 * reference's zarrita fixture (tests/golden/zarrita, i2 4x5x6 in 2x3x4 gzip
 * chunks) opened through zcg_array_meta_from_json, and a 2x3x3 and a 1x5x2
 * box read by ONE zcg_store_read_boxes_v call — what a binding's
 * ZarrNdarrayReader::read_ndarray does per box (ndarray.rs:153-268).  The
 * second box overhangs the array.  The boxes' bytes (each dense, C order, back
 * to back) are written to <out file>; the test compares them with the oracle.
 * Usage: boxes_v_c <store root> <out file> [device].  Prints "boxes_v_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_BOXES 2

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: boxes_v_c <store root> <out file> [device]\n"); return 2; }
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

    const uint64_t box_shapes[N_BOXES * 3] = {2, 3, 3, 1, 5, 2};
    const uint64_t offsets[N_BOXES * 3] = {1, 2, 3, 3, 1, 5};
    size_t at[N_BOXES + 1] = {0};
    for (int b = 0; b < N_BOXES; b++)
        at[b + 1] = at[b] + (size_t)(box_shapes[3 * b] * box_shapes[3 * b + 1] * box_shapes[3 * b + 2]) * sizeof(int16_t);
    uint8_t* buf = (uint8_t*)malloc(at[N_BOXES]);
    void* outs[N_BOXES];
    memset(buf, 0xA5, at[N_BOXES]);
    for (int b = 0; b < N_BOXES; b++) outs[b] = buf + at[b];

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_read_boxes_v(ctx, &m, root, "/seq/i2", box_shapes, offsets, outs, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_boxes_v: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f || fwrite(buf, 1, at[N_BOXES], f) != at[N_BOXES]) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    free(buf);
    printf("boxes_v_c: ok (%d boxes)\n", N_BOXES);
    return 0;
}
