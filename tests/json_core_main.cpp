// The data.json decode core (m6anet_amd/csrc/m6a_json.h) as a program of its own: tests/test_json_core.py builds it with ASan and UBSan
// and compares what it prints with tests/json_statement.py.  Every input is copied into an allocation of exactly its size first, so a
// read past `end` is a sanitizer report.
//   numbers FILE          a token per line -> its double as 16 hex digits, or "declined"
//   records FILE NORM     records (header line "tx \t pos \t n_reads \t bytes", then the bytes and a newline) -> a line each: the
//                         reason, and for "ok" the 7-mer and every value as hex
//   cuts FILE NORM        the same records cut at every length 0..bytes -> a line each: one letter per cut, 'a' + reason
//   dir DIR NORM MIN      data.info + data.json of a directory, rows with >= MIN reads -> "<sites> <declined>" and the declined ones
// NORM: a file of 5-mers, one per line, or "-" for no norm table.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "m6a_json.h"

using namespace m6a_json;

static uint64_t pack5(const char *k)
{
    uint64_t x = 0;
    for (int j = 0; j < 5; j++) x = x << 8 | (uint8_t)k[j];
    return x;
}

static std::vector<uint64_t> vocab_keys()
{
    std::vector<uint64_t> v;
    const std::string N = "ACGT", D = "AGT", R = "GA", H = "ACT";
    for (char a : N) for (char d : D) for (char r : R) for (char h : H) for (char b : N) {
        const char k7[7] = {a, d, r, 'A', 'C', h, b};
        for (int i = 0; i < 3; i++) v.push_back(pack5(k7 + i));
    }
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
    return v;
}

static std::string slurp(const char *path)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    std::stringstream ss;
    ss << f.rdbuf();
    return ss.str();
}

struct Norm { bool on = false; std::vector<uint64_t> keys; };
static Norm read_norm(const char *path)
{
    Norm n;
    if (!strcmp(path, "-")) return n;
    n.on = true;
    std::istringstream in(slurp(path));
    std::string line;
    while (std::getline(in, line))
        if (line.size() >= 5) n.keys.push_back(pack5(line.c_str()));
    std::sort(n.keys.begin(), n.keys.end());
    n.keys.erase(std::unique(n.keys.begin(), n.keys.end()), n.keys.end());
    return n;
}

struct Exact {                                // the bytes in an allocation of exactly their number
    uint8_t *p;
    size_t n;
    Exact(const char *s, size_t k) : p((uint8_t *)malloc(k ? k : 1)), n(k) { if (k) memcpy(p, s, k); }
    ~Exact() { free(p); }
};

static int walk_one(const char *bytes, size_t n, const std::string &tx, int64_t pos, int64_t n_reads, const Norm &norm, const std::vector<uint64_t> &voc,
                    std::vector<double> *vals, uint64_t *k7)
{
    Exact x(bytes, n);
    Exact t(tx.data(), tx.size());
    if (vals) vals->assign((size_t)n_reads * 10, 0.0);
    int na[3], va[3];
    return walk(x.p, x.p + n, t.p, (int64_t)t.n, pos, n_reads, norm.on ? norm.keys.data() : nullptr, (int)norm.keys.size(), voc.data(), (int)voc.size(),
                [&](int64_t r, int j, double v) { if (vals) (*vals)[(size_t)(10 * r + j)] = v; }, k7, na, va);
}

struct Rec { std::string tx; int64_t pos, n_reads; std::string bytes; };
static std::vector<Rec> read_records(const char *path)
{
    const std::string all = slurp(path);
    std::vector<Rec> out;
    size_t at = 0;
    while (at < all.size()) {
        const size_t nl = all.find('\n', at);
        if (nl == std::string::npos) break;
        std::istringstream head(all.substr(at, nl - at));
        Rec r;
        long long pos, nr, len;
        std::string tx;
        std::getline(head, tx, '\t');
        head >> pos >> nr >> len;
        r.tx = tx; r.pos = pos; r.n_reads = nr;
        r.bytes = all.substr(nl + 1, (size_t)len);
        at = nl + 1 + (size_t)len + 1;
        out.push_back(r);
    }
    return out;
}

int main(int argc, char **argv)
{
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint64_t> voc = vocab_keys();
    if (mode == "numbers") {
        std::istringstream in(slurp(argv[2]));
        std::string tok;
        while (std::getline(in, tok)) {
            Exact x(tok.data(), tok.size());
            double v = 0;
            const uint8_t *q = number(x.p, x.p + x.n, &v);
            if (!q || q != x.p + x.n) { puts("declined"); continue; }
            uint64_t b;
            memcpy(&b, &v, 8);
            printf("%016" PRIx64 "\n", b);
        }
        return 0;
    }
    if (argc < 4) return 2;
    const Norm norm = read_norm(argv[3]);
    if (mode == "records" || mode == "cuts") {
        for (const Rec &r : read_records(argv[2])) {
            if (mode == "cuts") {
                std::string line;
                for (size_t k = 0; k <= r.bytes.size(); k++) {
                    uint64_t k7;
                    std::vector<double> vals;
                    line += (char)('a' + walk_one(r.bytes.data(), k, r.tx, r.pos, r.n_reads, norm, voc, &vals, &k7));
                }
                puts(line.c_str());
                continue;
            }
            uint64_t k7 = 0;
            std::vector<double> vals;
            const int reason = walk_one(r.bytes.data(), r.bytes.size(), r.tx, r.pos, r.n_reads, norm, voc, &vals, &k7);
            fputs(reason_name(reason), stdout);
            if (!reason) {
                putchar(' ');
                for (int i = 0; i < 7; i++) putchar((char)(k7 >> (8 * (6 - i))));
                for (double v : vals) {
                    uint64_t b;
                    memcpy(&b, &v, 8);
                    printf(" %016" PRIx64, b);
                }
            }
            putchar('\n');
        }
        return 0;
    }
    if (mode == "dir" && argc >= 5) {
        const std::string dir = argv[2], json = slurp((dir + "/data.json").c_str());
        const long long min_reads = atoll(argv[4]);
        std::istringstream info(slurp((dir + "/data.info").c_str()));
        std::string line;
        std::getline(info, line);
        long long sites = 0, declined = 0;
        std::string report;
        while (std::getline(info, line)) {
            const size_t c = line.find(',');
            if (c == std::string::npos) continue;
            long long pos, a, b, nr;
            if (sscanf(line.c_str() + c + 1, "%lld,%lld,%lld,%lld", &pos, &a, &b, &nr) != 4) continue;
            if (nr < min_reads) continue;
            ++sites;
            int reason = JR_RANGE;
            uint64_t k7;
            if (a >= 0 && b <= (long long)json.size() && a < b) reason = walk_one(json.data() + a, (size_t)(b - a), line.substr(0, c), pos, nr, norm, voc, nullptr, &k7);
            if (reason) {
                ++declined;
                if (declined <= 10) report += line.substr(0, c) + ":" + std::to_string(pos) + " " + reason_name(reason) + "\n";
            }
        }
        printf("%lld %lld\n%s", sites, declined, report.c_str());
        return 0;
    }
    return 2;
}
