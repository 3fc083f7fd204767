// Stand-alone host program over csrc/jp2_parse.h with JP2_TAKE_TILES and the parity-aware lifting functions of csrc/jp2_t1.h (no HIP,
// no Python): tests/test_jp2_tiles_sanitized.py builds it with -fsanitize=address,undefined and runs it as a child process.
//   jp2_tiles_main LIST FLAGS [--pixels [SEGMENT]]
// LIST names one file per line; FLAGS is the `take` word of jp2_parse.  For each file it prints "status info[0..7] irreversible tiles
// reason-class", where reason-class is the reason with its blanks as underscores ("-" when empty); with --pixels a file of status 0 is
// also decoded on the host with the very functions the kernels run, tile-component by tile-component as the kernels walk them, and its
// RGB bytes are written to <file>.rgb.  The 9/7 lifting runs over windows of SEGMENT samples (even; default 256) with a halo of
// JP2_LIFT97_HALO a side, in exact-size heap blocks, so that a window that reads or trusts a sample it should not shows here.
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

static int cdivp(int a, int sh) { return (a + (1 << sh) - 1) >> sh; }

// one line of n samples, first canvas parity cas: src in sub-band order, dst interleaved.  T = int: 5/3, T = float: 9/7.
static void lift_line(const int* src, long long sstride, int* dst, long long dstride, int n, int cas, int) {
    // (an exact-size copy of the line, so that a read outside it is a heap overflow the sanitizer reports)
    std::unique_ptr<int[]> line(new int[(size_t)n]);
    for (int i = 0; i < n; ++i) line[(size_t)i] = src[i * sstride];
    for (int i = 0; i < n; ++i) dst[i * dstride] = jp2_lift_at(line.get(), 1, n, cas, i);
}
static void lift_line(const float* src, long long sstride, float* dst, long long dstride, int n, int cas, int segment) {
    std::unique_ptr<float[]> line(new float[(size_t)n]);
    for (int i = 0; i < n; ++i) line[(size_t)i] = src[i * sstride];
    for (int seg0 = 0; seg0 < n; seg0 += segment) {
        const int lo = std::max(0, seg0 - JP2_LIFT97_HALO), hi = std::min(n, seg0 + segment + JP2_LIFT97_HALO);
        std::unique_ptr<float[]> w(new float[(size_t)(hi - lo)]);
        for (int i = lo; i < hi; ++i) w[(size_t)(i - lo)] = jp2_lift97_load(line.get(), 1, n, i, cas);
        for (int s = 0; s < 4; ++s)
            for (int i = jp2_lift97_first(lo, s, cas); i < hi; i += 2) jp2_lift97_at(w.get(), 1, lo, hi, n, i, jp2_lift97_coef(s));
        for (int i = seg0; i < std::min(n, seg0 + segment); ++i) dst[i * dstride] = w[(size_t)(i - lo)];
    }
}

template <class T>
static void transform(std::vector<T>& a, const Jp2File& f, int segment) {
    const int W = f.width;
    const size_t npx = (size_t)W * f.height;
    std::vector<T> b(a.size(), (T)0);
    for (int c = 0; c < f.comps; ++c)
        for (const Jp2Tile& tile : f.tiles) {
            T* pa = a.data() + (size_t)c * npx + (size_t)(tile.y0 - f.y0) * W + (tile.x0 - f.x0);
            T* pb = b.data() + (size_t)c * npx + (size_t)(tile.y0 - f.y0) * W + (tile.x0 - f.x0);
            for (int r = 1; r <= f.levels; ++r) {
                const int sh = f.levels - r, rx0 = cdivp(tile.x0, sh), ry0 = cdivp(tile.y0, sh);
                const int rw = cdivp(tile.x1, sh) - rx0, rh = cdivp(tile.y1, sh) - ry0;
                if (rw <= 0 || rh <= 0) continue;
                for (int y = 0; y < rh; ++y) lift_line(pa + (size_t)y * W, 1, pb + (size_t)y * W, 1, rw, rx0 & 1, segment);
                for (int x = 0; x < rw; ++x) lift_line(pb + x, W, pa + x, W, rh, ry0 & 1, segment);
            }
        }
}

static std::vector<uint8_t> decode_pixels(const std::vector<uint8_t>& file, const Jp2File& f, int segment) {
    const int W = f.width, H = f.height;
    const size_t npx = (size_t)W * H;
    std::vector<int> ai(f.irreversible ? 0 : npx * f.comps, 0);
    std::vector<float> af(f.irreversible ? npx * f.comps : 0, 0.0f);
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
        if (K.x < 0 || K.y < 0 || K.x + K.w > W || K.y + K.h > H) { fprintf(stderr, "block outside its plane\n"); exit(3); }
        for (int y = 0; y < K.h; ++y)
            for (int x = 0; x < K.w; ++x) {
                const size_t at = (size_t)K.comp * npx + (size_t)(K.y + y) * W + K.x + x;
                if (f.irreversible) af[at] = jp2_t1_value_f(*S, y, x, K.hs); else ai[at] = jp2_t1_value(*S, y, x);
            }
    }
    std::vector<uint8_t> rgb(npx * 3);
    if (f.irreversible) {
        transform(af, f, segment);
        for (size_t i = 0; i < npx; ++i) {
            if (f.comps == 1) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = jp2_sample97(af[i]);
            else jp2_finish97(af[i], af[npx + i], af[2 * npx + i], f.mct, &rgb[3 * i]);
        }
    } else {
        transform(ai, f, segment);
        auto sample = [](int v) { v += 128; return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); };
        for (size_t i = 0; i < npx; ++i) {
            int r, g, b;
            if (f.comps == 1) {
                r = g = b = ai[i];
            } else if (f.mct) {
                const int y = ai[i], u = ai[npx + i], v = ai[2 * npx + i];
                g = y - ((u + v) >> 2); r = v + g; b = u + g;
            } else {
                r = ai[i]; g = ai[npx + i]; b = ai[2 * npx + i];
            }
            rgb[3 * i] = sample(r); rgb[3 * i + 1] = sample(g); rgb[3 * i + 2] = sample(b);
        }
    }
    return rgb;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s LIST FLAGS [--pixels [SEGMENT]]\n", argv[0]); return 2; }
    const unsigned flags = (unsigned)atoi(argv[2]);
    const bool pixels = argc > 3 && std::string(argv[3]) == "--pixels";
    const int segment = argc > 4 ? atoi(argv[4]) : 256;
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
        const int rc = jp2_parse(exact.get(), file.size(), &f, flags);
        std::string why = f.reason && f.reason[0] ? f.reason : "-";
        std::replace(why.begin(), why.end(), ' ', '_');
        printf("%d %d %d %d %d %d %d %d %d %d %d %s\n", rc, f.info[0], f.info[1], f.info[2], f.info[3], f.info[4], f.info[5], f.info[6], f.info[7],
               f.irreversible, (int)f.tiles.size(), why.c_str());
        if (rc == 0 && pixels) {
            const std::vector<uint8_t> rgb = decode_pixels(file, f, segment);
            std::ofstream out(path + ".rgb", std::ios::binary);
            out.write(reinterpret_cast<const char*>(rgb.data()), (std::streamsize)rgb.size());
        }
    }
    return 0;
}
