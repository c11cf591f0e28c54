/* A plain-C caller of the strided box write: a copy of the reference's zarrita
 * fixture (i2 4x5x6 in 2x3x4 gzip chunks) opened through
 * zcg_array_meta_from_json; two boxes of 2x2x3 samples, with steps 2,3,2 from
 * 0,1,0 and steps 1,2,2 from 2,0,1, are written by ONE
 * zcg_store_write_boxes_s call and read back by one zcg_store_read_boxes_s
 * call, which must return the values written.  zcg_regions_s_waves tells that
 * the two boxes share no sample.  The bytes read back (each box dense, C
 * order, back to back) are written to <out file>; the test also compares the
 * whole array with values it computes itself.  THE STORE IS MODIFIED: run it on
 * a copy.
 * Usage: boxes_sw_c <store root> <out file> [device].  Prints "boxes_sw_c: ok". */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "zchunk_gpu.h"

#define N_BOXES 2
#define N_EL 12 /* 2 x 2 x 3 samples */

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: boxes_sw_c <store root> <out file> [device]\n"); return 2; }
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

    const uint64_t box_shapes[N_BOXES * 3] = {2, 2, 3, 2, 2, 3};
    const uint64_t box_steps[N_BOXES * 3] = {2, 3, 2, 1, 2, 2};
    const uint64_t offsets[N_BOXES * 3] = {0, 1, 0, 2, 0, 1};
    int16_t in[N_BOXES][N_EL], back[N_BOXES][N_EL];
    const void* ins[N_BOXES];
    void* outs[N_BOXES];
    for (int b = 0; b < N_BOXES; b++) {
        for (int i = 0; i < N_EL; i++) in[b][i] = (int16_t)(-1000 * (b + 1) - i);
        ins[b] = in[b];
        outs[b] = back[b];
    }
    memset(back, 0xA5, sizeof back);

    zcg_region r;
    memset(&r, 0, sizeof r);
    r.ndim = m.ndim;
    for (uint32_t d = 0; d < m.ndim; d++) { r.array_shape[d] = m.shape[d]; r.chunk_shape[d] = m.chunk_shape[d]; }
    uint32_t wave_of[N_BOXES];
    const uint32_t waves = zcg_regions_s_waves(&r, offsets, box_shapes, box_steps, N_BOXES, wave_of);
    if (waves != 1) { fprintf(stderr, "expected one wave, got %u\n", waves); return 1; }

    zcg_ctx* ctx = zcg_create(device);
    if (!ctx) { fprintf(stderr, "zcg_create(%d) failed\n", device); return 2; }
    st = zcg_store_write_boxes_s(ctx, &m, root, "/seq/i2", box_shapes, box_steps, offsets, ins, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_write_boxes_s: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    st = zcg_store_read_boxes_s(ctx, &m, root, "/seq/i2", box_shapes, box_steps, offsets, outs, N_BOXES, 0, 4);
    if (st != ZCG_OK) { fprintf(stderr, "zcg_store_read_boxes_s: %d %s\n", st, zcg_last_error(ctx)); return 1; }
    zcg_destroy(ctx);
    if (memcmp(in, back, sizeof in) != 0) { fprintf(stderr, "the boxes read back differ from the boxes written\n"); return 1; }

    f = fopen(argv[2], "wb");
    if (!f || fwrite(back, 1, sizeof back, f) != sizeof back) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fclose(f);
    printf("boxes_sw_c: ok (%d boxes, %u wave)\n", N_BOXES, waves);
    return 0;
}
