// Stand-alone host program over csrc/jp2_parse.h (with the irreversible option) and the 9/7 functions of csrc/jp2_t1.h (no HIP, no
// Python): tests/test_jp2_irreversible_sanitized.py builds it with -fsanitize=address,undefined and runs it as a child process.
//   jp2_irreversible_main LIST [--pixels [SEGMENT]]
// LIST names one file per line.  For each it prints "status info[0..7] irreversible"; with --pixels a 9/7 file of status 0 is also
// decoded on the host with the very functions the kernels run (tier 1, dequantisation, lifting, colour, rounding) and its RGB bytes
// are written to <file>.rgb.  The lifting runs as the kernels run it: over windows of SEGMENT samples of a line (even; default 256)
// with a halo of JP2_LIFT97_HALO samples a side, so that a window that reads or trusts a sample it should not shows here.
#include <algorithm>
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

// the inverse 9/7 transform of one line of n samples: src in sub-band order, dst interleaved
static void lift_line(const float* src, long long sstride, float* dst, long long dstride, int n, int segment) {
    for (int seg0 = 0; seg0 < n; seg0 += segment) {
        const int lo = std::max(0, seg0 - JP2_LIFT97_HALO), hi = std::min(n, seg0 + segment + JP2_LIFT97_HALO);
        // (an exact-size window, so that a step outside it is a heap overflow the sanitizer reports)
        std::unique_ptr<float[]> w(new float[(size_t)(hi - lo)]);
        for (int i = lo; i < hi; ++i) w[(size_t)(i - lo)] = jp2_lift97_load(src, sstride, n, i);
        for (int s = 0; s < 4; ++s)
            for (int i = lo + (s & 1); i < hi; i += 2) jp2_lift97_at(w.get(), 1, lo, hi, n, i, jp2_lift97_coef(s));
        for (int i = seg0; i < std::min(n, seg0 + segment); ++i) dst[i * dstride] = w[(size_t)(i - lo)];
    }
}

static std::vector<uint8_t> decode_pixels(const std::vector<uint8_t>& file, const Jp2File& f, int segment) {
    const int W = f.width, H = f.height;
    const size_t npx = (size_t)W * H;
    std::vector<float> a(npx * f.comps, 0.0f), b(npx * f.comps, 0.0f);
    auto S = std::make_unique<Jp2T1State>();
    std::vector<uint8_t> data;
    for (const Jp2Block& K : f.blocks) {
        if (!K.passes) continue;
        data.clear();
        for (int s = K.seg_head; s >= 0; s = f.segs[(size_t)s].next)
            data.insert(data.end(), file.begin() + (long)f.segs[(size_t)s].off, file.begin() + (long)(f.segs[(size_t)s].off + f.segs[(size_t)s].len));
        *S = Jp2T1State{};
        jp2_t1_tables(*S, 0, 1);
        std::unique_ptr<uint8_t[]> exact(new uint8_t[data.size() ? data.size() : 1]);
        std::copy(data.begin(), data.end(), exact.get());
        jp2_t1_walk(*S, exact.get(), (uint32_t)data.size(), K.w, K.h, K.orient, K.mb - K.zbp, K.passes);
        for (int y = 0; y < K.h; ++y)
            for (int x = 0; x < K.w; ++x) a[(size_t)K.comp * npx + (size_t)(K.y + y) * W + K.x + x] = jp2_t1_value_f(*S, y, x, K.hs);
    }
    for (int c = 0; c < f.comps; ++c) {
        float* pa = a.data() + (size_t)c * npx;
        float* pb = b.data() + (size_t)c * npx;
        for (int r = 1; r <= f.levels; ++r) {
            const int rw = cdiv(W, 1 << (f.levels - r)), rh = cdiv(H, 1 << (f.levels - r));
            for (int y = 0; y < rh; ++y) lift_line(pa + (size_t)y * W, 1, pb + (size_t)y * W, 1, rw, segment);
            for (int x = 0; x < rw; ++x) lift_line(pb + x, W, pa + x, W, rh, segment);
        }
    }
    std::vector<uint8_t> rgb(npx * 3);
    for (size_t i = 0; i < npx; ++i) {
        if (f.comps == 1) {
            rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = jp2_sample97(a[i]);
        } else {
            jp2_finish97(a[i], a[npx + i], a[2 * npx + i], f.mct, &rgb[3 * i]);
        }
    }
    return rgb;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s LIST [--pixels [SEGMENT]]\n", argv[0]); return 2; }
    const bool pixels = argc > 2 && std::string(argv[2]) == "--pixels";
    const int segment = argc > 3 ? atoi(argv[3]) : 256;
    if (segment < 2 || (segment & 1)) { fprintf(stderr, "SEGMENT must be even and at least 2\n"); return 2; }
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
        const int rc = jp2_parse(exact.get(), file.size(), &f, true);
        printf("%d %d %d %d %d %d %d %d %d %d\n", rc, f.info[0], f.info[1], f.info[2], f.info[3], f.info[4], f.info[5], f.info[6], f.info[7], f.irreversible);
        if (rc == 0 && pixels && f.irreversible) {
            const std::vector<uint8_t> rgb = decode_pixels(file, f, segment);
            std::ofstream out(path + ".rgb", std::ios::binary);
            out.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)rgb.size());
        }
    }
    return 0;
}
