// Adler-32 of a file's bytes, computed with zcg_adler.h the way the GPU kernels
// do (tests/test_adler_host.py compares with zlib.adler32):
//   adler_host comb FILE    64 lanes per wave, 4 waves; wave w takes the 16 KiB
//                           slices w, w + 4, ...; in a slice lane l takes the 16
//                           bytes at l * 16 of every 1 KiB tile (a short last
//                           tile padded with zero pieces); lanes, then slices,
//                           fold by adler_add: adler32_verify's walk
//   adler_host block FILE   256 lanes over 4 KiB tiles of the whole file:
//                           zlib_adler32's walk
//   adler_host lane FILE    every 16-byte piece into ONE lane, which is closed
//                           and reopened each ADLER_LANE_MAX_PIECES pieces: the
//                           deferred-modulo bound itself
// Prints the checksum as 8 hex digits.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../zarr_amd/csrc/zcg_adler.h"

using namespace zcg;

// the piece at stream position p of the n bytes (zero past the end)
static void load_piece(const std::vector<uint8_t>& d, uint64_t p, uint32_t x[4]) {
    uint8_t b[16] = {0};
    for (uint64_t j = 0; j < 16 && p + j < d.size(); j++) b[j] = d[p + j];
    for (int i = 0; i < 4; i++)
        x[i] = (uint32_t)b[4 * i] | ((uint32_t)b[4 * i + 1] << 8) | ((uint32_t)b[4 * i + 2] << 16) |
               ((uint32_t)b[4 * i + 3] << 24);
}

// lanes `nl` wide over [off, end): lane l takes l * 16 of every nl * 16 byte tile
static uint32_t comb(const std::vector<uint8_t>& d, uint64_t off, uint64_t end, uint32_t nl) {
    const uint64_t D = d.size(), tile = (uint64_t)nl * 16;
    const uint64_t ntile = (end - off + tile - 1) / tile;
    uint32_t sum = 0;
    for (uint32_t l = 0; l < nl && ntile; l++) {
        AdlerLane al = adler_lane_open();
        uint64_t p = off + (uint64_t)l * 16;
        for (uint64_t k = 0; k < ntile; k++, p += tile) {
            uint32_t x[4] = {0, 0, 0, 0};
            if (p < end) load_piece(d, p, x);
            adler_lane_piece(al, x[0], x[1], x[2], x[3]);
        }
        p -= tile;
        sum = adler_add(sum, adler_lane_close(al, (int64_t)D - (int64_t)p - 16, (uint32_t)tile));
    }
    return sum;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) d.insert(d.end(), buf, buf + k);
    fclose(f);
    const uint64_t D = d.size();
    uint32_t sum = 0;
    if (!strcmp(argv[1], "comb")) {
        const uint64_t slice = 16384;
        for (uint64_t off = 0; off < D; off += slice) sum = adler_add(sum, comb(d, off, off + slice < D ? off + slice : D, 64));
    } else if (!strcmp(argv[1], "block")) {
        sum = comb(d, 0, D, 256);
    } else if (!strcmp(argv[1], "lane")) {
        AdlerLane al = adler_lane_open();
        uint32_t held = 0;
        uint64_t p = 0;
        for (; p < D; p += 16) {
            if (held == ADLER_LANE_MAX_PIECES) {  // the lane is full: its last piece sits at p - 16
                sum = adler_add(sum, adler_lane_close(al, (int64_t)D - (int64_t)p, 16));
                al = adler_lane_open();
                held = 0;
            }
            uint32_t x[4];
            load_piece(d, p, x);
            adler_lane_piece(al, x[0], x[1], x[2], x[3]);
            held++;
        }
        if (held) sum = adler_add(sum, adler_lane_close(al, (int64_t)D - (int64_t)p, 16));
    } else {
        return 2;
    }
    printf("%08x\n", adler_finish(sum, D));
    return 0;
}
