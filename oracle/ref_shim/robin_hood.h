// Stand-in for robin_hood.h (robin-hood-hashing), which the reference's kmer_searcher.cpp includes but
// the reference checkout does not vendor.  The program uses robin_hood::unordered_map / unordered_set as
// plain maps and sets only (count, at, operator[], insert().second, iteration), so the standard containers
// serve.  The one visible difference is the order of the indices inside an output.bin record, which the
// reference leaves unspecified; the comparisons in tests/ sort each record first.
#pragma once
#include <algorithm>
#include <limits>
#include <unordered_map>
#include <unordered_set>

namespace robin_hood {
template <typename Key, typename T, typename Hash = std::hash<Key>, typename KeyEqual = std::equal_to<Key>>
using unordered_map = std::unordered_map<Key, T, Hash, KeyEqual>;
template <typename Key, typename Hash = std::hash<Key>, typename KeyEqual = std::equal_to<Key>>
using unordered_set = std::unordered_set<Key, Hash, KeyEqual>;
}  // namespace robin_hood
