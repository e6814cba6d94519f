// _stdorder.cpp -- the permutations this C++ standard library produces for the calls ripples/main.cpp makes:
// std::shuffle with std::default_random_engine(0) (:249) and std::sort by an int key (combine_intervals, :133-164).
// Compiled at test time (tests/stdorder.py); the restatement in tests/ripples_ref.py uses them to reproduce the reference's
// branch order and its tie order among equal keys.
#include <algorithm>
#include <cstdint>
#include <random>
#include <vector>

extern "C" void std_shuffle(int64_t n, int64_t *out) {
    std::vector<int64_t> v(n);
    for (int64_t i = 0; i < n; i++) v[i] = i;
    std::shuffle(v.begin(), v.end(), std::default_random_engine(0));
    for (int64_t i = 0; i < n; i++) out[i] = v[i];
}

namespace {
struct Item { int64_t key, idx; bool operator<(const Item &o) const { return key < o.key; } };
}

extern "C" void std_sort_by_key(int64_t n, const int64_t *key, int64_t *perm) {
    std::vector<Item> v(n);
    for (int64_t i = 0; i < n; i++) v[i] = Item{key[i], perm[i]};
    std::sort(v.begin(), v.end());
    for (int64_t i = 0; i < n; i++) perm[i] = v[i].idx;
}
