// Stand-alone host program over csrc/blob_check.h (no HIP, no Python): tests/test_blob_check_sanitized.py builds it with and without
// -fsanitize=address,undefined and runs it as a child process.
//   blob_main check KIND BASE RECIPES   KIND: det | rec | cls | svtr.  For every mutant of the recipe file (tests/blob_cases.py
//                                       serialise) one line "status<TAB>reason<TAB>tensor" from blob_parse + check_blob
//   blob_main spec KIND BASE            the tensor list check_blob holds BASE to: "name<TAB>dtype<TAB>required<TAB>dims ..." (class count: -1)
// The base blob is read once into a working buffer with room for the longest tail.  A mutant's patches are applied in place and undone
// after use; what lies past the mutant's end is poisoned while it is checked (sanitized build), so a read past the end is reported
// as it would be past a heap block.  A truncated mutant is checked in a heap copy of exactly its length, and an odd-address mutant
// in a copy that starts one byte into its block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <memory>
#include <string>
#include <vector>

#include "blob_check.h"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION(p, n)
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION(p, n)
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

struct Patch { uint64_t off; std::vector<uint8_t> data; };
struct Tail { std::vector<uint8_t> data; uint64_t zeros; };
struct Mutant { std::string label; bool odd; int64_t trunc; std::vector<Patch> patches; std::vector<Tail> tail; };

static bool read_file(const char* path, std::vector<uint8_t>* out) {
    std::ifstream in(path, std::ios::binary | std::ios::ate);
    if (!in) return false;
    out->resize((size_t)in.tellg());
    in.seekg(0);
    in.read(reinterpret_cast<char*>(out->data()), (std::streamsize)out->size());
    return (bool)in;
}

struct Reader {
    const std::vector<uint8_t>& b; size_t off = 0; bool ok = true;
    template <class T> T get() {
        T v = T();
        if (b.size() - off < sizeof(T)) { ok = false; return v; }
        memcpy(&v, b.data() + off, sizeof(T)); off += sizeof(T);
        return v;
    }
    std::vector<uint8_t> bytes(size_t n) {
        if (b.size() - off < n) { ok = false; return {}; }
        std::vector<uint8_t> v(b.begin() + (std::ptrdiff_t)off, b.begin() + (std::ptrdiff_t)(off + n)); off += n;
        return v;
    }
};

static bool read_mutants(const char* path, std::vector<Mutant>* out) {
    std::vector<uint8_t> file;
    if (!read_file(path, &file)) return false;
    Reader r{file};
    const uint32_t n = r.get<uint32_t>();
    for (uint32_t i = 0; i < n && r.ok; ++i) {
        Mutant m;
        const std::vector<uint8_t> label = r.bytes(r.get<uint16_t>());
        m.label.assign(label.begin(), label.end());
        m.odd = r.get<uint8_t>() != 0;
        m.trunc = r.get<int64_t>();
        for (uint32_t k = r.get<uint32_t>(); k > 0 && r.ok; --k) {
            Patch p; p.off = r.get<uint64_t>();
            p.data = r.bytes(r.get<uint32_t>());
            m.patches.push_back(std::move(p));
        }
        for (uint32_t k = r.get<uint32_t>(); k > 0 && r.ok; --k) {
            Tail t; const uint32_t len = r.get<uint32_t>();
            t.zeros = r.get<uint64_t>();
            t.data = r.bytes(len);
            m.tail.push_back(std::move(t));
        }
        out->push_back(std::move(m));
    }
    return r.ok && r.off == file.size();
}

static int kind_of(const char* s) {
    const char* names[4] = {"det", "rec", "cls", "svtr"};
    for (int i = 0; i < 4; ++i) if (!strcmp(s, names[i])) return i;
    return -1;
}

static void report(BlobKind kind, const uint8_t* blob, size_t n) {
    BlobMap m;
    BlobError e;
    const bool ok = blob_parse(blob, n, &m, &e) && check_blob(kind, m, &e);
    printf("%d\t%s\t%s\n", ok ? 0 : 1, ok ? "" : e.reason.c_str(), ok ? "" : e.tensor.c_str());
}

int main(int argc, char** argv) {
    const int kind = argc >= 4 ? kind_of(argv[2]) : -1;
    if (kind < 0 || (strcmp(argv[1], "check") && strcmp(argv[1], "spec")) || (!strcmp(argv[1], "check") && argc < 5)) {
        fprintf(stderr, "usage: %s check KIND BASE RECIPES | spec KIND BASE\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> base;
    if (!read_file(argv[3], &base)) { fprintf(stderr, "cannot read %s\n", argv[3]); return 2; }
    if (!strcmp(argv[1], "spec")) {
        BlobMap m;
        BlobError e;
        std::vector<BlobSpec> spec;
        if (!blob_parse(base.data(), base.size(), &m, &e) || !blob_spec((BlobKind)kind, m, &spec, &e)) { fprintf(stderr, "%s %s\n", e.reason.c_str(), e.tensor.c_str()); return 1; }
        for (const BlobSpec& s : spec) {
            printf("%s\t%d\t%d\t", s.name.c_str(), s.dtype, (int)s.required);
            for (size_t d = 0; d < s.dims.size(); ++d) printf("%s%d", d ? " " : "", s.dims[d]);
            printf("\n");
        }
        return 0;
    }
    std::vector<Mutant> mutants;
    if (!read_mutants(argv[4], &mutants)) { fprintf(stderr, "cannot read %s\n", argv[4]); return 2; }
    size_t cap = base.size();
    for (const Mutant& m : mutants) {
        size_t n = base.size();
        for (const Tail& t : m.tail) n += t.data.size() + (size_t)t.zeros;
        if (n > cap) cap = n;
        for (const Patch& p : m.patches)
            if (p.off > base.size() || p.data.size() > base.size() - p.off) { fprintf(stderr, "patch outside the base: %s\n", m.label.c_str()); return 2; }
    }
    cap = (cap + 15) / 16 * 16;
    uint8_t* work = static_cast<uint8_t*>(malloc(cap));
    if (!work) { fprintf(stderr, "out of memory\n"); return 2; }
    memcpy(work, base.data(), base.size());
    for (const Mutant& m : mutants) {
        std::vector<Patch> undo;
        for (const Patch& p : m.patches) {
            undo.push_back(Patch{p.off, std::vector<uint8_t>(work + p.off, work + p.off + p.data.size())});
            memcpy(work + p.off, p.data.data(), p.data.size());
        }
        size_t n = base.size();
        for (const Tail& t : m.tail) {
            if (!t.data.empty()) memcpy(work + n, t.data.data(), t.data.size());
            n += t.data.size();
            memset(work + n, 0, (size_t)t.zeros);
            n += (size_t)t.zeros;
        }
        if (m.trunc >= 0 && (size_t)m.trunc <= n) {
            std::unique_ptr<uint8_t[]> cut(new uint8_t[(size_t)m.trunc ? (size_t)m.trunc : 1]);
            if (m.trunc) memcpy(cut.get(), work, (size_t)m.trunc);
            report((BlobKind)kind, cut.get(), (size_t)m.trunc);
        } else if (m.odd) {
            std::unique_ptr<uint8_t[]> shifted(new uint8_t[n + 1]);
            uint8_t* p = shifted.get() + 1;   // (operator new[] returns an even address)
            memcpy(p, work, n);
            report((BlobKind)kind, p, n);
        } else {
            POISON(work + n, cap - n);
            report((BlobKind)kind, work, n);
            UNPOISON(work + n, cap - n);
        }
        for (size_t i = undo.size(); i-- > 0;) memcpy(work + undo[i].off, undo[i].data.data(), undo[i].data.size());
    }
    free(work);
    return 0;
}
