// The slot list of one stream-pool call, checked on the host before anything is launched: shared by the GRU pool (stream_pool.cpp) and
// the Transformer pool (vit_stream.cpp).  The stamp table says which call last named a slot, so the duplicate check allocates nothing.
#pragma once
#include "host_common.h"

#include <algorithm>
#include <cstdint>
#include <vector>

// the vote records of a pool, for what serves both pool types (stream_feed.cpp); each is defined beside its pool's struct
const PoolGeom* stream_pool_geom(const prego_stream_pool* p);
const PoolGeom* vit_stream_pool_geom(const prego_vit_stream_pool* p);
const PoolGeom* decode_pool_geom(const prego_decode_pool* p);      // decode_pool.cpp: the records of the decode pool's committed labels
// what the slot images need on top (stream_image.cpp): a pool's stamp table, its block, the Transformer pool's ring, and of a feed the pool
// it was created over and its cursor words
struct SlotStamps;
struct PoolBlock { const char* base; size_t bytes; };
SlotStamps* stream_pool_stamps(prego_stream_pool* p);
SlotStamps* vit_stream_pool_stamps(prego_vit_stream_pool* p);
PoolBlock stream_pool_block(const prego_stream_pool* p);
PoolBlock vit_stream_pool_block(const prego_vit_stream_pool* p);
const VitRing* vit_stream_pool_ring(const prego_vit_stream_pool* p);
const PoolGeom* stream_pool_feed_pool(const prego_stream_pool_feed* f);
const FeedGeom* stream_pool_feed_geom(const prego_stream_pool_feed* f);

struct SlotStamps {
  std::vector<unsigned> stamp;           // [capacity]: the call that last named the slot
  unsigned call = 0;
};

// n in 1..min(256, capacity), every slot inside the pool and named once; 0 = fine, else PREGO_EINVAL with a message
static inline int check_slot_list(SlotStamps& st, int capacity, const char* who, int n, const int32_t* slots) {
  const int n_max = capacity < kPoolMaxActive ? capacity : kPoolMaxActive;
  if (n < 1 || n > n_max)
    return prego_fail_(PREGO_EINVAL, "%s: %d slots (1..%d per call: at most %d, pool capacity %d)", who, n, n_max, kPoolMaxActive, capacity);
  if (!slots) return prego_fail_(PREGO_EINVAL, "%s: slots is NULL", who);
  for (int i = 0; i < n; ++i)
    if (slots[i] < 0 || slots[i] >= capacity)
      return prego_fail_(PREGO_EINVAL, "%s: slots[%d] = %d is outside the pool (capacity %d)", who, i, slots[i], capacity);
  if (++st.call == 0) {                                       // the counter wrapped: old stamps could alias
    std::fill(st.stamp.begin(), st.stamp.end(), 0u);
    st.call = 1;
  }
  for (int i = 0; i < n; ++i) {
    if (st.stamp[(size_t)slots[i]] == st.call) return prego_fail_(PREGO_EINVAL, "%s: slot %d is named twice", who, slots[i]);
    st.stamp[(size_t)slots[i]] = st.call;
  }
  return 0;
}
