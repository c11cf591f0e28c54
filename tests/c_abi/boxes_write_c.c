/* A plain-C caller of the batched box write: a copy of the reference's
 * zarrita fixture (i2 4x5x6 in 2x3x4 gzip chunks) opened through
 * zcg_array_meta_from_json, four 2x3x3 boxes written by ONE
 * zcg_store_write_boxes call (chunk keys, the reads of partly covered chunks,
 * GPU decode, scatter, encode and the file writes all inside it) — what a
 * binding's ZarrNdarrayWriter::write_ndarray does per box (ndarray.rs:276-385)
 * — and read back by one zcg_store_read_boxes call.  Boxes 1 and 2 overlap
 * (the later one wins), the last box overhangs the array.  Box b holds the
 * values 1000*(b+1) + i (i = index in the dense C-order box).  The bytes read
 * back (dense, C order, back to back) are written to <out file>; the test
 * compares them, and the store's chunk files, with the oracle.
 * Usage: boxes_write_c <store root> <out file> [device].  The store is
 * modified.  Prints "boxes_write_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_BOXES 4
#define BOX_ELEMS (2 * 3 * 3)

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: boxes_write_c <store root> <out file> [device]\n"); return 2; }
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

    const uint64_t box_shape[3] = {2, 3, 3};
    const uint64_t offsets[N_BOXES * 3] = {0, 0, 0, 1, 2, 3, 2, 1, 2, 3, 4, 5};
    const size_t box_bytes = BOX_ELEMS * sizeof(int16_t);
    int16_t* in = (int16_t*)malloc(N_BOXES * box_bytes);
    uint8_t* back = (uint8_t*)malloc(N_BOXES * box_bytes);
    const void* ins[N_BOXES];
    void* outs[N_BOXES];
    memset(back, 0xA5, N_BOXES * box_bytes);
    for (int b = 0; b < N_BOXES; b++) {
        for (int i = 0; i < BOX_ELEMS; i++) in[b * BOX_ELEMS + i] = (int16_t)(1000 * (b + 1) + i);
        ins[b] = in + b * BOX_ELEMS;
        outs[b] = back + (size_t)b * box_bytes;
    }

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_write_boxes(ctx, &m, root, "/seq/i2", box_shape, offsets, ins, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_write_boxes: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    st = zcg_store_read_boxes(ctx, &m, root, "/seq/i2", box_shape, offsets, outs, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_boxes: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f || fwrite(back, 1, N_BOXES * box_bytes, f) != N_BOXES * box_bytes) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    free(in);
    free(back);
    printf("boxes_write_c: ok (%d boxes)\n", N_BOXES);
    return 0;
}
