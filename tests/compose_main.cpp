// Stand-alone host program over csrc/compose.h: the table check (compose_params_ok) and the per-pixel function (compose_pixel) the
// kernel of lumina_ocr_page_compose runs, compiled for the host so that the sanitizers see them (tests/test_compose_sanitized.py).
//
//   compose_main LIST      LIST: one "table-file output-file" pair per line
// A table file is int32 {n, H, W, m}, then per layer int32 {page, kind, x0, y0, x1, y1, flip, fill, w, h, mw, mh, has_src, has_mask}
// followed by the source (w * h * 3 bytes, when has_src) and the mask (mw * mh * 3 bytes, when has_mask).  Every image is read into
// an allocation of exactly its size, so a sample index outside it is a report.  Per table one line is printed: "ok", or "rejected: "
// and the reason; the pages ([n][H][W][3]) of an accepted table go to the output file.  Exit status 0 unless a file is malformed.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "compose.h"

static bool read_exact(FILE* f, void* p, size_t n) { return n == 0 || fread(p, 1, n, f) == n; }

static int one(const std::string& in, const std::string& out) {
    FILE* f = fopen(in.c_str(), "rb");
    if (!f) return 2;
    int32_t head[4];
    if (!read_exact(f, head, sizeof(head))) { fclose(f); return 2; }
    const int n = head[0], H = head[1], W = head[2], m = head[3];
    if (m < 0 || m > 4096) { fclose(f); return 2; }
    std::vector<ComposeLayer> table((size_t)m);
    std::vector<std::unique_ptr<uint8_t[]>> images;
    for (int i = 0; i < m; ++i) {
        int32_t q[14];
        if (!read_exact(f, q, sizeof(q))) { fclose(f); return 2; }
        ComposeLayer& L = table[(size_t)i];
        L.page = q[0]; L.kind = q[1]; L.x0 = q[2]; L.y0 = q[3]; L.x1 = q[4]; L.y1 = q[5]; L.flip = q[6]; L.fill = q[7];
        L.w = q[8]; L.h = q[9]; L.mw = q[10]; L.mh = q[11]; L.src = nullptr; L.mask = nullptr;
        for (int k = 0; k < 2; ++k) {
            if (!q[12 + k]) continue;
            const int64_t w = k ? L.mw : L.w, h = k ? L.mh : L.h;
            if (w < 0 || h < 0 || w * h > (1 << 26)) { fclose(f); return 2; }
            const size_t bytes = (size_t)(w * h * 3);
            images.emplace_back(new uint8_t[bytes ? bytes : 1]);
            if (!read_exact(f, images.back().get(), bytes)) { fclose(f); return 2; }
            (k ? L.mask : L.src) = images.back().get();
        }
    }
    fclose(f);
    if (const char* why = compose_params_why(table.data(), m, n, H, W)) {
        printf("rejected: %s\n", why);
        return 0;
    }
    if (compose_params_ok(table.data(), m, n, H, W) != true) return 2;
    std::vector<uint8_t> pages((size_t)n * H * W * 3);
    size_t at = 0;
    for (int p = 0; p < n; ++p)
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                uint32_t c = 0xffffff;
                for (int i = 0; i < m; ++i)
                    if (table[(size_t)i].page == p) c = compose_pixel(c, table[(size_t)i], x, y);
                pages[at++] = (uint8_t)c; pages[at++] = (uint8_t)(c >> 8); pages[at++] = (uint8_t)(c >> 16);
            }
    FILE* g = fopen(out.c_str(), "wb");
    if (!g) return 2;
    const bool ok = pages.empty() || fwrite(pages.data(), 1, pages.size(), g) == pages.size();
    fclose(g);
    if (!ok) return 2;
    printf("ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: compose_main LIST\n"); return 2; }
    std::ifstream list(argv[1]);
    std::string line;
    while (std::getline(list, line)) {
        std::istringstream ss(line);
        std::string in, out;
        if (!(ss >> in >> out)) continue;
        const int rc = one(in, out);
        if (rc) { fprintf(stderr, "%s: malformed table file\n", in.c_str()); return rc; }
    }
    // the sample map at the limits the check admits: the widest span, the largest images, both ends
    const int spans[3] = {1, 65535, 2 * COMPOSE_MAX_COORD}, sizes[3] = {1, 40000, 65535};
    for (int s : spans)
        for (int w : sizes)
            for (int d : {0, s / 2, s - 1}) {
                const int64_t want = ((2 * (int64_t)d + 1) * w) / (2 * (int64_t)s);
                if (compose_map(d, s, w) != (int)want || want < 0 || want >= w) {
                    fprintf(stderr, "compose_map(%d, %d, %d)\n", d, s, w);
                    return 3;
                }
            }
    return 0;
}
