// The slot image of a stream pool (prego_stream_pool_snapshot / _restore; kernels: stream_image.hip, host side: stream_image.cpp): one
// slot of either pool type as position-independent data.  The layout and the validity rule stand here once, for the kernels, the host
// code and (by the same words and bit values) the Python model prego_amd/stream_pool.py: image_fault.
// An image is image_words 32-bit words, a multiple of 64 (256 bytes), the same for every slot of a pool:
//   tag    [16]           magic | version | kind | dim | window_size | n_classes | vote window | max_events |
//                         frames | head | fill | feed cursor word | 0 | 0 | 0 | 0
//                         kind 1 = GRU pool (dim = hid, window_size 0, head = fill = 0), kind 2 = Transformer pool (dim = embedding_dim)
//   state  [state_words]  GRU: the fp32 state row [hid]; Transformer: the ring [window_size][dim] fp32 at its physical rows, rows that
//                         fill does not cover as zeros (the covered rows are [0, fill): head = frames mod T, fill = min(frames, T))
//   record [rec_words]    the slot's vote record as the pool keeps it (stream_pool.hip): frames | last vote + 1 | n_events | overflow |
//                         counts[ncls_pad] | event_id[max_events] | event_start[max_events]
//   0 ..                  up to the next multiple of 64 words
// state_words and rec_words are multiples of 4, so every part starts 16-byte aligned.  The same stream gives the same bytes whatever
// slot it lived in: nothing of the image depends on a slot number, an address or what the slot held before.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define POOL_IMAGE_HD __host__ __device__
#else
#define POOL_IMAGE_HD
#endif

constexpr int kPoolImageMagic = 0x474d4950;        // "PIMG", little endian
constexpr int kPoolImageVersion = 1;
constexpr int kPoolImageGru = 1, kPoolImageVit = 2;
constexpr int kPoolImageTagWords = 16;
constexpr int kPoolImageRecHeader = 4;             // kPoolRecHeader (kernels.h)
enum PoolImageTag {
  kTagMagic = 0, kTagVersion, kTagKind, kTagDim, kTagWindowSize, kTagClasses, kTagVoteWindow, kTagMaxEvents,      // 0..7: the geometry
  kTagFrames, kTagHead, kTagFill, kTagCursor                                                                      // 12..15 spare, zero
};
constexpr unsigned kPoolImageCursorCount = 0x3fffffffu;      // the feed cursor's delivered count (stream_feed.hip)

// one bit per clause of the validity rule: the words of `status` after a restore
constexpr int kImageFaultGeometry = 1;      // tag words 0..7 differ from the pool's geometry
constexpr int kImageFaultFrames = 2;        // frames < 0, or the record's frames differs from the tag's
constexpr int kImageFaultEvents = 4;        // n_events outside 0..max_events
constexpr int kImageFaultVote = 8;          // last vote + 1 outside 0..n_classes
constexpr int kImageFaultOverflow = 16;     // overflow word outside 0..3
constexpr int kImageFaultCounter = 32;      // a counter outside 0..vote window
constexpr int kImageFaultRing = 64;         // Transformer pool: head != frames mod window_size or fill != min(frames, window_size)
constexpr int kImageFaultCursor = 128;      // the cursor's delivered count is above n_events

struct PoolImageDims {
  int kind, dim, window_size, ncls, ncls_pad, vote_window, max_events;
  int state_words, rec_words, image_words;
};

POOL_IMAGE_HD inline PoolImageDims pool_image_dims(int kind, int dim, int window_size, int ncls, int ncls_pad, int vote_window, int max_events,
                                                   int rec_words) {
  PoolImageDims d{kind, dim, window_size, ncls, ncls_pad, vote_window, max_events, 0, rec_words, 0};
  d.state_words = kind == kPoolImageVit ? window_size * dim : dim;
  d.image_words = (kPoolImageTagWords + d.state_words + rec_words + 63) / 64 * 64;
  return d;
}

// the word the geometry clause wants at tag[k], k in 0..7
POOL_IMAGE_HD inline int pool_image_geometry_word(const PoolImageDims& d, int k) {
  return k == kTagMagic ? kPoolImageMagic : k == kTagVersion ? kPoolImageVersion : k == kTagKind ? d.kind : k == kTagDim ? d.dim
       : k == kTagWindowSize ? (d.kind == kPoolImageVit ? d.window_size : 0) : k == kTagClasses ? d.ncls
       : k == kTagVoteWindow ? d.vote_window : d.max_events;
}

// every clause but the counters': tag = the image's 16 tag words, hdr = the first 4 words of its record
POOL_IMAGE_HD inline int pool_image_fault_words(const PoolImageDims& d, const int* tag, const int* hdr) {
  int f = 0;
  for (int k = 0; k < 8; ++k)
    if (tag[k] != pool_image_geometry_word(d, k)) f |= kImageFaultGeometry;
  const int frames = tag[kTagFrames], n_events = hdr[2];
  if (frames < 0 || hdr[0] != frames) f |= kImageFaultFrames;
  if (n_events < 0 || n_events > d.max_events) f |= kImageFaultEvents;
  if (hdr[1] < 0 || hdr[1] > d.ncls) f |= kImageFaultVote;
  if (hdr[3] < 0 || hdr[3] > 3) f |= kImageFaultOverflow;
  if (d.kind == kPoolImageVit && frames >= 0) {                // negative frames: the frames clause has refused the image already
    const int fill = frames < d.window_size ? frames : d.window_size;
    if (tag[kTagHead] != frames % d.window_size || tag[kTagFill] != fill) f |= kImageFaultRing;
  }
  if ((int)((unsigned)tag[kTagCursor] & kPoolImageCursorCount) > (n_events < 0 ? 0 : n_events)) f |= kImageFaultCursor;
  return f;
}

// the counters' clause for one counter word
POOL_IMAGE_HD inline int pool_image_fault_counter(const PoolImageDims& d, int count) {
  return (count < 0 || count > d.vote_window) ? kImageFaultCounter : 0;
}

// THE RULE: 0 = the image may be restored into a pool of geometry d, else a bit per failed clause.  rec = the image's record words
// (4 + ncls_pad of them are read).  The restore kernel evaluates the same two functions, its lanes sharing the counters.
POOL_IMAGE_HD inline int pool_image_fault(const PoolImageDims& d, const int* tag, const int* rec) {
  int f = pool_image_fault_words(d, tag, rec);
  for (int c = 0; c < d.ncls_pad; ++c) f |= pool_image_fault_counter(d, rec[kPoolImageRecHeader + c]);
  return f;
}
