// A bounded first-in-first-out cache of owned entries: the one shape of the context's device-table caches.
// A caller looks an entry up with find(); on a miss it builds a new one in a local std::unique_ptr and hands it over with publish()
// only once the entry is complete, so a build that returns early leaves the cache as it was and its entry destroys itself.
// No HIP here: the host test-suite compiles this header on its own.
#pragma once
#include <cstddef>
#include <memory>
#include <utility>
#include <vector>

template <class T>
class TableCache {
public:
    explicit TableCache(size_t cap) : cap_(cap) {}
    size_t size() const { return entries_.size(); }
    // the first entry pred accepts, or null
    template <class Pred>
    T *find(Pred pred) const {
        for (const std::unique_ptr<T> &e : entries_)
            if (pred(*e)) return e.get();
        return nullptr;
    }
    // append `entry`.  A full cache first calls drain() -- the caller's wait for whatever may still read the oldest entry; a nonzero return
    // is handed back with the cache unchanged -- and drops that entry.
    template <class Drain>
    int publish(std::unique_ptr<T> entry, Drain drain) {
        if (entries_.size() >= cap_) {
            if (int rc = drain()) return rc;
            entries_.erase(entries_.begin());
        }
        entries_.push_back(std::move(entry));
        return 0;
    }
    void clear() { entries_.clear(); }

private:
    size_t cap_;
    std::vector<std::unique_ptr<T>> entries_;
};
