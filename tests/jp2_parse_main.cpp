// Stand-alone host program over csrc/jp2_parse.h and csrc/jp2_t1.h (no HIP, no Python): tests/test_jp2_parser_sanitized.py builds it
// with -fsanitize=address,undefined and runs it over the damage sweep.
//   jp2_parse_main LIST [--pixels]
// LIST names one file per line.  For each it prints "status info[0..7]"; with --pixels a file of status 0 is also decoded on the host
// with the very functions the kernels run (tier 1, lifting) and its RGB bytes are written to <file>.rgb.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "jp2_parse.h"
#include "jp2_t1.h"

static std::vector<uint8_t> read_file(const std::string& path, bool* ok) {
    std::ifstream in(path, std::ios::binary);
    *ok = (bool)in;
    return std::vector<uint8_t>((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
}

static int cdiv(int a, int b) { return (a + b - 1) / b; }

static std::vector<uint8_t> decode_pixels(const std::vector<uint8_t>& file, const Jp2File& f) {
    const int W = f.width, H = f.height;
    const size_t npx = (size_t)W * H;
    std::vector<int> a(npx * f.comps, 0), b(npx * f.comps, 0);
    auto S = std::make_unique<Jp2T1State>();
    std::vector<uint8_t> data;
    for (const Jp2Block& K : f.blocks) {
        if (!K.passes) continue;
        data.clear();
        for (int s = K.seg_head; s >= 0; s = f.segs[(size_t)s].next)
            data.insert(data.end(), file.begin() + (long)f.segs[(size_t)s].off, file.begin() + (long)(f.segs[(size_t)s].off + f.segs[(size_t)s].len));
        *S = Jp2T1State{};
        jp2_t1_tables(*S, 0, 1);
        // (an exact-size copy, so that a read past the block's data is a heap overflow the sanitizer reports)
        std::unique_ptr<uint8_t[]> exact(new uint8_t[data.size() ? data.size() : 1]);
        std::copy(data.begin(), data.end(), exact.get());
        jp2_t1_walk(*S, exact.get(), (uint32_t)data.size(), K.w, K.h, K.orient, K.mb - K.zbp, K.passes);
        for (int y = 0; y < K.h; ++y)
            for (int x = 0; x < K.w; ++x) a[(size_t)K.comp * npx + (size_t)(K.y + y) * W + K.x + x] = jp2_t1_value(*S, y, x);
    }
    for (int c = 0; c < f.comps; ++c) {
        int* pa = a.data() + (size_t)c * npx;
        int* pb = b.data() + (size_t)c * npx;
        for (int r = 1; r <= f.levels; ++r) {
            const int rw = cdiv(W, 1 << (f.levels - r)), rh = cdiv(H, 1 << (f.levels - r));
            for (int y = 0; y < rh; ++y)
                for (int k = 0; k < (rw + 1) / 2; ++k) {
                    pb[(size_t)y * W + 2 * k] = jp2_lift_even(pa + (size_t)y * W, 1, rw, k);
                    if (2 * k + 1 < rw) pb[(size_t)y * W + 2 * k + 1] = jp2_lift_odd(pa + (size_t)y * W, 1, rw, k);
                }
            for (int x = 0; x < rw; ++x)
                for (int k = 0; k < (rh + 1) / 2; ++k) {
                    pa[(size_t)(2 * k) * W + x] = jp2_lift_even(pb + x, W, rh, k);
                    if (2 * k + 1 < rh) pa[(size_t)(2 * k + 1) * W + x] = jp2_lift_odd(pb + x, W, rh, k);
                }
        }
    }
    std::vector<uint8_t> rgb(npx * 3);
    auto sample = [](int v) { v += 128; return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
    for (size_t i = 0; i < npx; ++i) {
        int r, g, bl;
        if (f.comps == 1) {
            r = g = bl = a[i];
        } else if (f.mct) {
            const int y = a[i], u = a[npx + i], v = a[2 * npx + i];
            g = y - ((u + v) >> 2); r = v + g; bl = u + g;
        } else {
            r = a[i]; g = a[npx + i]; bl = a[2 * npx + i];
        }
        rgb[3 * i] = sample(r); rgb[3 * i + 1] = sample(g); rgb[3 * i + 2] = sample(bl);
    }
    return rgb;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s LIST [--pixels]\n", argv[0]); return 2; }
    const bool pixels = argc > 2 && std::string(argv[2]) == "--pixels";
    std::ifstream list(argv[1]);
    if (!list) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::string path;
    while (std::getline(list, path)) {
        if (path.empty()) continue;
        bool ok = false;
        const std::vector<uint8_t> file = read_file(path, &ok);
        if (!ok) { fprintf(stderr, "cannot read %s\n", path.c_str()); return 2; }
        // (an exact-size heap copy: a read past the end of the file is a heap overflow the sanitizer reports)
        std::unique_ptr<uint8_t[]> exact(new uint8_t[file.size() ? file.size() : 1]);
        std::copy(file.begin(), file.end(), exact.get());
        Jp2File f;
        const int rc = jp2_parse(exact.get(), file.size(), &f);
        printf("%d %d %d %d %d %d %d %d %d\n", rc, f.info[0], f.info[1], f.info[2], f.info[3], f.info[4], f.info[5], f.info[6], f.info[7]);
        if (rc == 0 && pixels) {
            const std::vector<uint8_t> rgb = decode_pixels(file, f);
            std::ofstream out(path + ".rgb", std::ios::binary);
            out.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)rgb.size());
        }
    }
    return 0;
}
