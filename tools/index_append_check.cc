// index_append_check.cc -- host check of the digest index's growth after its
// build (csrc/index_map.hpp: insert over a base, skipped entries, rehash_slot),
// run one entry after the other on plain slot arrays, against a std::map of
// the lowest admitted position of every digest.
//
// A model index is what rt_index.hip keeps: a table with room for `capacity`
// rows, slots_for(capacity) slots, `size` positions handed out.  Random
// sequences of
//   create   m digests, inserted in a random order;
//   append   k digests behind the last position, each with a skip byte: all k
//            rows are written first (the device copies them before the kernel
//            starts), then the entries that are not skipped are inserted.  The
//            append kernel's lanes arrive in any order, so every call is
//            inserted in several orders (all of them for k <= 4), each on its
//            own copy of the slot array, and every order must answer alike;
//   growth   a larger capacity: a fresh slot array filled by rehash_slot from
//            the old one, its slots visited in several orders;
//   lookup   every digest ever given (admitted, skipped, duplicated) and misses.
// A tenth of a call repeats earlier digests, a few repeat digests of the same
// call, and some repeat digests that were only ever skipped.  Checked after
// every step: each answer equals the map's (a digest that was only skipped is
// kEmpty), one slot per admitted distinct digest, every slot holds the lowest
// admitted position of its digest, never a position >= size.
// Chains: calls whose digests share their first 8 bytes (one home), at homes in
// the middle and at the last slots so that the chain wraps, appended in several
// calls with duplicates in later calls, across a growth (which gives the chain
// another home).
//
// Stand-alone: c++ -std=c++17 tools/index_append_check.cc (make tools;
// make index-append-check-asan for the same under ASan + UBSan).
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <numeric>
#include <string>
#include <vector>

#include "../congestion-control-with-bittorren_amd/csrc/index_map.hpp"

using namespace s1ix;
using Digest = std::array<uint32_t, kWords>;

namespace {
uint64_t g_rng = 0x0fedcba987654321ull;
uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
uint64_t rnd() { return g_rng = splitmix64(g_rng); }

Digest random_digest() {
    Digest d;
    for (auto& w : d) w = static_cast<uint32_t>(rnd());
    return d;
}
Digest with_prefix(uint32_t w0, uint32_t w1) {
    Digest d = random_digest();
    d[0] = w0;
    d[1] = w1;
    return d;
}
std::string key(const Digest& d) { return std::string(reinterpret_cast<const char*>(d.data()), 20); }

void prefix_with_home(uint64_t slots, uint32_t want, uint32_t* w0, uint32_t* w1) {
    for (;;) {
        *w0 = static_cast<uint32_t>(rnd());
        *w1 = static_cast<uint32_t>(rnd());
        if (home(*w0, *w1, static_cast<uint32_t>(slots - 1)) == want) return;
    }
}

uint64_t g_appends, g_orders, g_growths, g_lookups, g_wrapped;

[[noreturn]] void die(const char* what, size_t a, size_t b) {
    fprintf(stderr, "index_append_check: %s (%zu, %zu)\n", what, a, b);
    exit(1);
}

struct Model {
    std::vector<Digest> table;   // rows [0, size); capacity rows of room
    uint64_t capacity = 0;
    std::vector<uint32_t> slots;
    std::map<std::string, uint32_t> lowest;  // admitted digests only
    std::vector<Digest> given;               // every digest ever given, skipped ones included

    uint32_t mask() const { return static_cast<uint32_t>(slots.size() - 1); }
    const uint32_t* words() const { return table.empty() ? nullptr : table[0].data(); }

    // every answer and the array's shape, for a slot array of the current table
    void check(const std::vector<uint32_t>& arr, const char* when) {
        if (arr.size() != slots_for(capacity) || table.size() > capacity) die("slot count", arr.size(), capacity);
        const PlainSlots S{const_cast<uint32_t*>(arr.data())};
        size_t held = 0;
        for (uint32_t v : arr) {
            if (v == kEmpty) continue;
            if (v >= table.size()) die("position outside the table", v, table.size());
            auto it = lowest.find(key(table[v]));
            if (it == lowest.end()) die("a slot holds a digest that was never admitted", v, 0);
            if (it->second != v) die("slot does not hold the lowest admitted position", v, it->second);
            ++held;
        }
        if (held != lowest.size()) die(when, held, lowest.size());
        if (2 * held > arr.size()) die("more than half full", held, arr.size());
        for (size_t i = 0; i < given.size(); ++i) {
            auto it = lowest.find(key(given[i]));
            const uint32_t want = it == lowest.end() ? kEmpty : it->second;
            if (lookup(S, mask(), words(), given[i].data()) != want) die("lookup", i, want);
            ++g_lookups;
        }
        for (int i = 0; i < 20; ++i) {
            const Digest q = i % 2 && !given.empty() ? with_prefix(given[rnd() % given.size()][0],
                                                                   given[rnd() % given.size()][1])
                                                     : random_digest();
            auto it = lowest.find(key(q));
            if (lookup(S, mask(), words(), q.data()) != (it == lowest.end() ? kEmpty : it->second)) die("miss", i, 0);
            ++g_lookups;
        }
    }

    void create(const std::vector<Digest>& rows) {
        table = rows;
        capacity = rows.size();
        slots.assign(slots_for(capacity), kEmpty);
        lowest.clear();
        given = rows;
        std::vector<uint32_t> order(rows.size());
        std::iota(order.begin(), order.end(), 0u);
        for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
        for (uint32_t p : order) (void)insert(PlainSlots{slots.data()}, mask(), words(), p);
        for (uint32_t p = 0; p < rows.size(); ++p) lowest.emplace(key(rows[p]), p);
        check(slots, "create: slots held != distinct digests");
    }

    // the capacity check of the device form is the caller's
    void append(const std::vector<Digest>& rows, const std::vector<uint8_t>& skip) {
        const uint32_t base = static_cast<uint32_t>(table.size()), k = static_cast<uint32_t>(rows.size());
        if (base + k > capacity) die("append past the capacity", base + k, capacity);
        table.insert(table.end(), rows.begin(), rows.end());  // the rows before any insert
        given.insert(given.end(), rows.begin(), rows.end());
        std::vector<uint32_t> order;
        for (uint32_t i = 0; i < k; ++i) {
            if (skip[i]) continue;
            order.push_back(base + i);
            lowest.emplace(key(rows[i]), base + i);  // keeps an earlier, lower position
        }
        std::vector<uint32_t> result;
        auto run = [&](const std::vector<uint32_t>& ord) {
            std::vector<uint32_t> arr = slots;
            for (uint32_t p : ord) {
                const Probe r = insert(PlainSlots{arr.data()}, mask(), words(), p);
                if (r.visited < 1 || r.visited > table.size()) die("probe length", p, r.visited);
                g_wrapped += r.wrapped;
            }
            check(arr, "append: slots held != admitted distinct digests");
            result = arr;
            ++g_orders;
        };
        if (order.size() <= 4) {
            do run(order);
            while (std::next_permutation(order.begin(), order.end()));
        } else {
            run(order);
            std::reverse(order.begin(), order.end());
            run(order);
            for (int rep = 0; rep < 3; ++rep) {
                for (size_t i = order.size(); i > 1; --i) std::swap(order[i - 1], order[rnd() % i]);
                run(order);
            }
        }
        slots = result;
        ++g_appends;
    }

    void grow(uint64_t to) {
        if (to <= capacity) return;
        const std::vector<uint32_t> old = slots;
        capacity = to;
        std::vector<uint32_t> visit(old.size());
        std::iota(visit.begin(), visit.end(), 0u);
        for (int rep = 0; rep < 3; ++rep) {
            slots.assign(slots_for(capacity), kEmpty);
            for (uint32_t s : visit)
                rehash_slot(PlainSlots{const_cast<uint32_t*>(old.data())}, s, PlainSlots{slots.data()}, mask(), words());
            check(slots, "growth: slots held != admitted distinct digests");
            if (rep == 0) std::reverse(visit.begin(), visit.end());
            else
                for (size_t i = visit.size(); i > 1; --i) std::swap(visit[i - 1], visit[rnd() % i]);
        }
        ++g_growths;
    }
};

// k digests for a call: fresh ones, a tenth repeated from what was given before
// (admitted or only skipped), a few repeated from the call itself.
std::vector<Digest> call_digests(const Model& M, size_t k) {
    std::vector<Digest> rows;
    for (size_t i = 0; i < k; ++i) {
        const uint64_t r = rnd() % 20;
        if (r < 2 && !M.given.empty()) rows.push_back(M.given[rnd() % M.given.size()]);
        else if (r == 2 && i) rows.push_back(rows[rnd() % i]);
        else rows.push_back(random_digest());
    }
    return rows;
}

std::vector<uint8_t> skip_mask(size_t k, int kind) {
    std::vector<uint8_t> s(k, 0);
    for (auto& b : s) b = kind == 0 ? 0 : kind == 1 ? 1 : (rnd() % 4 == 0 ? static_cast<uint8_t>(1 + rnd() % 255) : 0);
    return s;
}

void random_sequence(size_t m, int steps) {
    Model M;
    std::vector<Digest> rows;
    for (size_t p = 0; p < m; ++p) rows.push_back(p && rnd() % 8 == 0 ? rows[rnd() % p] : random_digest());
    M.create(rows);
    for (int step = 0; step < steps; ++step) {
        static const size_t sizes[] = {0, 1, 1, 2, 3, 4, 7, 63, 64, 65, 200};
        const size_t k = sizes[rnd() % (sizeof sizes / sizeof *sizes)];
        if (M.table.size() + k > M.capacity)  // the host form: at least doubled; sometimes an exact reserve
            M.grow(rnd() % 3 ? std::max<uint64_t>(M.table.size() + k, 2 * M.capacity) : M.table.size() + k);
        M.append(call_digests(M, k), skip_mask(k, static_cast<int>(rnd() % 5)));
    }
}

// 200 digests of one home appended in four calls of 50 behind `m` random
// digests, then a duplicate of each in later calls, then a growth.
void chain_sequence(size_t m, bool at_the_end) {
    Model M;
    std::vector<Digest> rows;
    for (size_t p = 0; p < m; ++p) rows.push_back(random_digest());
    M.create(rows);
    M.grow(m + 400);
    const uint64_t slots = slots_for(M.capacity);
    uint32_t w0, w1;
    prefix_with_home(slots, at_the_end ? static_cast<uint32_t>(slots - 20) : static_cast<uint32_t>(slots / 2), &w0, &w1);
    std::vector<Digest> chain;
    for (int i = 0; i < 200; ++i) chain.push_back(with_prefix(w0, w1));
    const uint64_t wrapped_before = g_wrapped;
    for (int c = 0; c < 4; ++c) {
        std::vector<Digest> part(chain.begin() + 50 * c, chain.begin() + 50 * (c + 1));
        std::vector<uint8_t> skip(50, 0);
        if (c == 1) skip[7] = skip[8] = 1;  // two links that join the set only with their duplicate
        M.append(part, skip);
    }
    if (at_the_end != (g_wrapped > wrapped_before)) die("chain wrap", at_the_end, g_wrapped - wrapped_before);
    for (int c = 0; c < 4; ++c) {
        std::vector<Digest> part(chain.begin() + 50 * c, chain.begin() + 50 * (c + 1));
        std::reverse(part.begin(), part.end());
        M.append(part, skip_mask(50, c == 0 ? 0 : 2));
    }
    M.grow(4 * M.capacity);
    M.append(call_digests(M, 64), skip_mask(64, 2));
}
}  // namespace

int main() {
    for (size_t m : {0, 1, 3, 4, 5, 100})
        for (int rep = 0; rep < 12; ++rep) random_sequence(m, 25);
    for (size_t m : {0, 1000})
        for (bool at_the_end : {false, true}) chain_sequence(m, at_the_end);
    // a skipped digest stays unanswered across a growth and answers the later position afterwards
    {
        Model M;
        M.create({random_digest(), random_digest(), random_digest()});
        const Digest d = random_digest();
        M.grow(4);
        M.append({d}, {1});
        if (M.lowest.count(key(d))) die("skipped digest admitted", 0, 0);
        M.grow(16);
        M.append({M.table[0], d, d}, {1, 0, 0});
        if (M.lowest.at(key(d)) != 5 || M.lowest.at(key(M.table[0])) != 0) die("later position", 0, 0);
    }
    printf("index_append_check: %llu appends in %llu orders, %llu growths, %llu lookups: ok\n",
           static_cast<unsigned long long>(g_appends), static_cast<unsigned long long>(g_orders),
           static_cast<unsigned long long>(g_growths), static_cast<unsigned long long>(g_lookups));
    return 0;
}
