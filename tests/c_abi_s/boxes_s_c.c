/* A plain-C caller of the strided box read: the reference's zarrita fixture
 * (tests/golden/zarrita, i2 4x5x6 in 2x3x4 gzip chunks) opened through
 * zcg_array_meta_from_json, and two strided boxes read by ONE
 * zcg_store_read_boxes_s call: 2x2x3 samples with steps 2,3,2 from 0,1,0, and
 * 2x3x2 samples with steps 1,2,4 from 2,0,1.  The second box's first step
 * dimension and last sample column reach the array's edge.  zcg_region_s_chunks
 * tells how many chunk files each box needs.  The boxes' bytes (each dense,
 * C order, back to back) are written to <out file>; the test compares them
 * with values it computes itself.
 * Usage: boxes_s_c <store root> <out file> [device].  Prints "boxes_s_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_BOXES 2

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: boxes_s_c <store root> <out file> [device]\n"); return 2; }
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

    const uint64_t box_shapes[N_BOXES * 3] = {2, 2, 3, 2, 3, 2};
    const uint64_t box_steps[N_BOXES * 3] = {2, 3, 2, 1, 2, 4};
    const uint64_t offsets[N_BOXES * 3] = {0, 1, 0, 2, 0, 1};
    size_t at[N_BOXES + 1] = {0};
    for (int b = 0; b < N_BOXES; b++)
        at[b + 1] = at[b] + (size_t)(box_shapes[3 * b] * box_shapes[3 * b + 1] * box_shapes[3 * b + 2]) * sizeof(int16_t);
    uint8_t* buf = (uint8_t*)malloc(at[N_BOXES]);
    void* outs[N_BOXES];
    memset(buf, 0xA5, at[N_BOXES]);
    for (int b = 0; b < N_BOXES; b++) outs[b] = buf + at[b];

    /* the chunks each box touches, out of its hull's grid range */
    zcg_region r;
    memset(&r, 0, sizeof r);
    r.ndim = m.ndim;
    for (uint32_t d = 0; d < m.ndim; d++) { r.array_shape[d] = m.shape[d]; r.chunk_shape[d] = m.chunk_shape[d]; }
    uint64_t touched[N_BOXES], range[N_BOXES];
    for (int b = 0; b < N_BOXES; b++) {
        uint64_t lo[ZCG_MAX_DIMS], n[ZCG_MAX_DIMS];
        touched[b] = zcg_region_s_chunks(&r, offsets + 3 * b, box_shapes + 3 * b, box_steps + 3 * b, lo, n, NULL);
        range[b] = n[0] * n[1] * n[2];
    }

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_read_boxes_s(ctx, &m, root, "/seq/i2", box_shapes, box_steps, offsets, outs, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_boxes_s: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);

    f = fopen(argv[2], "wb");
    if (!f || fwrite(buf, 1, at[N_BOXES], f) != at[N_BOXES]) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    free(buf);
    printf("boxes_s_c: ok (%d boxes, chunks %llu/%llu %llu/%llu)\n", N_BOXES, (unsigned long long)touched[0],
           (unsigned long long)range[0], (unsigned long long)touched[1], (unsigned long long)range[1]);
    return 0;
}
