// Stand-alone host program over csrc/jbig2_parse.h and the functions of csrc/jbig2_dec.h that the jb2_generic kernel runs (no HIP, no
// Python): tests/test_jbig2_parse_sanitized.py builds it with -fsanitize=address,undefined and runs it as a child process.
//   jbig2_main LIST [--general]
// LIST names one page per line: "<stream file> <globals file or ->".  For each it prints "status info[0..7] mmr decoded"; a page of
// status 0 without MMR regions (mmr = 0) and of at most MAX_PIXELS pixels (a damaged height can be anything) is also decoded
// (decoded = 1) with the very functions the kernel runs, row by row as the kernel drives them, and its bits (one byte a pixel,
// 1 = black) are written to <stream file>.bits.  The T.6 line stages of an MMR region are device code
// (ccitt_lines.h) and are not run here.  --general: every region takes the general path (contexts from their definition), also where
// its AT pixels are nominal: the two paths must give the same bits.
// Every buffer is an exact-size heap block, so that a step outside it is a heap overflow the sanitizer reports.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "jbig2_dec.h"
#include "jbig2_parse.h"

constexpr long long MAX_PIXELS = 1ll << 22;

static std::vector<uint8_t> read_file(const std::string& path, bool* ok) {
    std::ifstream in(path, std::ios::binary);
    *ok = (bool)in;
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static std::unique_ptr<uint8_t[]> exact_copy(const uint8_t* d, size_t n) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[n ? n : 1]);
    if (n) memcpy(p.get(), d, n);
    return p;
}

// one region as jb2_generic decodes it -> its plane, jb2_plane_words(w) words a row
static std::unique_ptr<uint32_t[]> decode_region(const Jb2Region& r, const uint8_t* data, int rows, bool general) {
    const int W = (int)r.w, pw = jb2_plane_words(W), rw = jb2_row_words(W);
    const std::unique_ptr<uint8_t[]> z = exact_copy(data, r.len);
    std::unique_ptr<uint8_t[]> cx(new uint8_t[(size_t)1 << jb2_context_bits(r.tmpl)]());
    std::unique_ptr<uint32_t[]> live[3], plane(new uint32_t[(size_t)pw * rows]());
    for (auto& l : live) l.reset(new uint32_t[(size_t)rw]());
    uint32_t mq[47];
    for (int i = 0; i < 47; ++i) mq[i] = jp2_mq_states[i];
    Jp2Mq m;
    m.cx[0] = m.cx[1] = m.cx[2] = 0;
    jp2_mq_init(m, z.get(), r.len);
    int ltp = 0;
    for (int y = 0; y < rows; ++y) {
        uint32_t* r0 = live[y % 3].get();
        const uint32_t* r1 = live[(y + 2) % 3].get();
        const uint32_t* r2 = live[(y + 1) % 3].get();
        std::fill(r0, r0 + rw, 0u);
        if (r.tpgd) ltp ^= jb2_sltp(m, mq, cx.get(), r.tmpl);
        if (!ltp) {
            const Jb2Rows rr{r0, r1, r2, plane.get(), pw, W, y};
            if (r.nominal && !general) jb2_row_nominal(m, mq, cx.get(), rr, r.tmpl);
            else jb2_row_general(m, mq, cx.get(), rr, r.tmpl, r.at);
        } else {
            std::copy(r1, r1 + pw, r0);
        }
        std::copy(r0, r0 + pw, plane.get() + (size_t)y * pw);
    }
    return plane;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s LIST [--general]\n", argv[0]); return 2; }
    const bool general = argc > 2 && std::string(argv[2]) == "--general";
    std::ifstream list(argv[1]);
    if (!list) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string line;
    while (std::getline(list, line)) {
        if (line.empty()) continue;
        std::istringstream parts(line);
        std::string path, gpath;
        parts >> path >> gpath;
        bool ok = false;
        const std::vector<uint8_t> file = read_file(path, &ok);
        if (!ok) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        std::vector<uint8_t> gfile;
        if (gpath != "-") {
            gfile = read_file(gpath, &ok);
            if (!ok) { fprintf(stderr, "cannot read %s\n", gpath.c_str()); return 2; }
        }
        const std::unique_ptr<uint8_t[]> s = exact_copy(file.data(), file.size()), g = exact_copy(gfile.data(), gfile.size());
        Jb2Page pg;
        const int rc = jbig2_parse(s.get(), file.size(), gpath != "-" ? g.get() : nullptr, gfile.size(), &pg);
        const int mmr = pg.info[4] > 0, W = pg.width, H = pg.height;
        const bool pixels = rc == 0 && !mmr && (long long)W * H <= MAX_PIXELS;
        printf("%d %d %d %d %d %d %d %d %d %d %d\n", rc, pg.info[0], pg.info[1], pg.info[2], pg.info[3], pg.info[4], pg.info[5], pg.info[6], pg.info[7], mmr,
               (int)pixels);
        if (!pixels) continue;
        std::vector<uint8_t> bits((size_t)W * H, (uint8_t)pg.default_pixel);
        for (const Jb2Region& r : pg.regions) {
            const int rows = (int)std::min<uint32_t>(r.h, (uint32_t)(H - (int)r.y)), pw = jb2_plane_words((int)r.w);
            const std::unique_ptr<uint32_t[]> plane = decode_region(r, (r.from_globals ? g.get() : s.get()) + r.off, rows, general);
            for (int y = 0; y < rows; ++y)
                for (int x = 0; x < (int)r.w && (int)r.x + x < W; ++x) {
                    const int src = (int)((plane[(size_t)y * pw + (x >> 5)] >> (x & 31)) & 1u);
                    uint8_t& dst = bits[(size_t)((int)r.y + y) * W + (int)r.x + x];
                    dst = (uint8_t)(r.op == 0 ? dst | src : r.op == 1 ? dst & src : r.op == 2 ? dst ^ src : r.op == 3 ? 1 - (dst ^ src) : src);
                }
        }
        std::ofstream out(path + ".bits", std::ios::binary);
        out.write(reinterpret_cast<const char*>(bits.data()), (std::streamsize)bits.size());
    }
    return 0;
}
