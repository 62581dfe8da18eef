/*
 * rudp.h — C ABI of librudp: batched Reliable-UDP wire codec on MI355X (gfx950).
 *
 * The reference (reotam5/Reliable-UDP) has no FFI: its boundary is the Python
 * class `Packet` in utils/packet.py:12-86 plus the module global
 * `custom_header` (utils/packet.py:3-10), imported by utils/reliableUDP.py:4
 * and proxy.py:10.  This header is the C boundary a maintainer binds (ctypes
 * stub in INTEGRATION.md) to move the per-packet work of that class onto the
 * GPU in batches.  Each entry point names the reference code it replaces.
 *
 * Wire format (utils/packet.py:3-10):
 *   byte 0-1  seq_num, big-endian u16
 *   byte 2-3  ack_num, big-endian u16
 *   byte 4    flags: bit7 SYN, bit6 ACK, bit5 FIN, bits4-0 `offset`
 *   RUDP_LAYOUT_RUDP7 only:
 *   byte 5-6  checksum, big-endian u16
 *   then the payload bytes.
 * Checksum (build-defined; the reference has none): RFC 1071 one's-complement
 * of the one's-complement sum of the frame taken as big-endian 16-bit words
 * with the checksum field (rudp7) zero and an odd tail zero-padded.  In the
 * rudp5 layout the frame carries no checksum field; the value is returned as
 * a sideband u16 per packet.  A decode verifies by recomputing that value and
 * comparing it with the carried one (the in-band field, or the sideband
 * entry), so a frame that carries 0xFFFF where the checksum is 0x0000, or the
 * reverse, is RUDP_OK_BAD_CSUM.
 *
 * Conventions
 *  - Buffers are caller-owned; the library never allocates or frees them.
 *  - Device (d_*) pointers are HIP device memory on `device`; calls are
 *    asynchronous on `hip_stream` (a hipStream_t, NULL = legacy default).
 *  - The *_host variants take host pointers and are synchronous.
 *  - Return 0 on success or a negative code (RUDP_E*); the message for the
 *    calling thread is available from rudp_last_error().
 *  - Reentrant and thread-safe: the only global state is mutex-guarded
 *    per-device caches (the *_host staging pipeline, the stream-ordered
 *    scratch pool, the call temporaries).  A call's device temporaries (scan
 *    sums, tile records, dedup hashes, offset-check partials) are kept per
 *    (device, stream), shared by all host threads: a call holds its stream's
 *    set while it enqueues (calls on one stream serialize on the host, as
 *    they do on the GPU) and the next call on that stream reuses it (stream
 *    order keeps them safe).  Nothing is held per host thread, so short-lived
 *    threads leave nothing behind; at most 64 streams per device keep a set.
 *    Once a device has 64, every call records an event behind its work as
 *    it ends, and a call on a 65th stream takes the least recently used set
 *    that has one, its own stream waiting for that event
 *    (hipStreamWaitEvent: stream order, no host wait, no device
 *    synchronize); with none, the call uses temporaries allocated and freed
 *    in stream order.  A temporary grown past 64 MiB is freed when its call
 *    ends.  Under stream capture the temporaries are allocated and freed
 *    inside the graph.  While another thread holds a GLOBAL-mode stream
 *    capture (hipStreamCaptureModeGlobal), the HIP runtime refuses
 *    stream-ordered allocations and cross-stream event waits made outside
 *    the capture: a call that needs either -- one on a stream without a set
 *    once the device has 64, or whose temporaries must grow -- fails with
 *    RUDP_EHIP_BASE - hipError and a message naming the capture, having
 *    enqueued nothing; the capture is unaffected, and the call succeeds if
 *    repeated after the capture ends.  Calls on streams that already hold
 *    a large-enough set, and captures in thread-local or relaxed mode, are
 *    not affected.
 *    Every launch choice is fixed at its
 *    measured default; librudp.so exports exactly the functions below.  (The
 *    diagnostics build of the same sources, librudp_tools.so, adds non-ABI
 *    rudpx_* sweep knobs and timelines for tools/ and is not a product library.)
 */
#ifndef RUDP_H_
#define RUDP_H_

#include <stdint.h>

/* Every entry point is exported; librudp is built with hidden default
 * visibility, so nothing else of it (kernels' host stubs, internal C++) can
 * interpose on another library's symbols or be interposed on. */
#if defined(__GNUC__)
#define RUDP_API __attribute__((visibility("default")))
#else
#define RUDP_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RUDP_ABI_VERSION 8

/* Frame layouts: the value is the header length in bytes. */
#define RUDP_LAYOUT_RUDP5 5 /* reference-exact 5-byte header, checksum sideband */
#define RUDP_LAYOUT_RUDP7 7 /* {**custom_header, "checksum": 2}, checksum in-band */

/* Per-packet decode status written to d_ok. */
#define RUDP_OK_BAD_CSUM 0   /* checksum mismatch */
#define RUDP_OK_GOOD 1       /* checksum verified */
#define RUDP_OK_SHORT 2      /* frame shorter than the header */
#define RUDP_OK_UNVERIFIED 3 /* rudp5 decoded without a sideband checksum */
#define RUDP_OK_BAD_OFFSETS 4 /* variable-length decode: frame_off[i] > frame_off[i+1] or past the buffer */

/*
 * Status word of the sync-free variable-length calls (*_checked): written on
 * the device by the call itself, 0 when the batch is valid, else these bits.
 * Encode rejects the whole batch: with a non-zero status it writes no frames
 * and no checksums, and of d_frame_off only d_frame_off[n] (the total its scan
 * found); d_frame_off[0..n-1] are then unspecified.  Decode rejects frame by
 * frame: every frame whose pair of offsets is bad gets d_ok =
 * RUDP_OK_BAD_OFFSETS and nothing of it is read, every other frame is fully
 * decoded, and RUDP_ST_OFFSETS is set when any frame was rejected.
 */
#define RUDP_ST_LEN 1u        /* a len[i] > 65535 */
#define RUDP_ST_PAYLOAD 2u    /* packed: sum(len) != payload_bytes; gathered: payload outside the buffer */
#define RUDP_ST_FRAMES_CAP 4u /* sum(len) + n*layout > frames_cap */
#define RUDP_ST_OFFSETS 8u    /* frame_off decreasing, or outside [0, frames_bytes] */
#define RUDP_ST_PAYLOAD_CAP 16u /* gather: the kept payloads need more than payload_cap bytes */
#define RUDP_ST_PACKETS_CAP 32u /* segment: the message makes more than max_packets packets */
#define RUDP_ST_RANK 64u        /* gather_ordered: a rank at or above the count that is not RUDP_RANK_NONE */
#define RUDP_ST_CARRY_CAP 128u  /* receive_window: the pending frames need more than carry_cap bytes */

/* Entry points added within an ABI version, for C callers to test. */
#define RUDP_HAS_SEGMENT_UTF8 1 /* rudp_segment_utf8 */
#define RUDP_HAS_ACCEPT_INORDER 1 /* rudp_payload_chars, rudp_accept_inorder */
#define RUDP_HAS_ACCEPT_WINDOW 1 /* rudp_accept_window, rudp_gather_ordered */

/* Error codes (negative errno values, HIP errors offset by -1000). */
#define RUDP_EINVAL (-22)
#define RUDP_ENOMEM (-12)
#define RUDP_ENOTSUP (-95)
#define RUDP_EHIP_BASE (-1000) /* returned as RUDP_EHIP_BASE - hipError_t */

/*
 * A batch of packets to frame: the SoA header table plus payload bytes.
 * Fixed-length batches (rudp_encode): payload is n*payload_len contiguous
 * bytes and len/payload_off are NULL.  Variable-length batches
 * (rudp_encode_varlen): len[i] payload bytes of packet i (<= 65535) start at
 * payload[payload_off[i]], or, with payload_off NULL, the payloads are packed
 * back to back in packet order; payload_len is then a hint of the typical
 * payload length (0 = unknown/tiny) that picks lanes per packet, never the
 * result.
 *   seq   -> custom_header["seq_num"]  (utils/packet.py:4)
 *   ack   -> custom_header["ack_num"]  (utils/packet.py:5)
 *   flags -> header byte 4 verbatim: syn/ack/fin/offset (utils/packet.py:6-9)
 */
typedef struct rudp_batch {
  uint64_t n;
  uint32_t payload_len;
  uint32_t reserved;
  const uint16_t* seq;
  const uint16_t* ack;
  const uint8_t* flags;
  const uint8_t* payload;
  const uint32_t* len;          /* variable-length batches: payload bytes per packet */
  const uint64_t* payload_off;  /* variable-length batches: payload start, or NULL = packed */
} rudp_batch;

/*
 * Frame + checksum a device-resident batch.
 * Replaces, per packet, the encode sequence of utils/reliableUDP.py:53-61
 * (Packet(); set_header_field x2..4; set_payload; to_byte) i.e.
 * utils/packet.py:13-16, :43-57, :60-65, :76-81.
 * d_frames: n*(payload_len+layout) bytes.  d_csum_or_null: n u16 (rudp5
 * sideband; for rudp7 it receives a copy of the in-band value).
 * The fixed-length tile takes payload_len % 16 == 0, payload_len <= 4096
 * and 16-byte aligned d_frames and payload; any other shape (the reference's
 * 1-4 B datagrams, any length, unaligned views) runs the variable-length tile
 * kernels with implicit offsets (one launch, no offset array) with identical
 * results.  An unaligned buffer is read from the 16-byte boundary at or below
 * its first byte to the one at or above its last (the same aligned 16-byte
 * blocks, hence pages); nothing outside d_frames / d_csum is written.
 */
RUDP_API int rudp_encode(const rudp_batch* in, uint8_t* d_frames, uint16_t* d_csum_or_null,
                int layout, int device, void* hip_stream);

/*
 * Parse + verify a device-resident batch of fixed-length frames.
 * Replaces, per packet, utils/reliableUDP.py:118-123 / :67-73
 * (Packet(data); get_header_field x N; get_payload), i.e.
 * utils/packet.py:16, :29-40, :68-73.
 * Fixed-length frames: d_frame_off_or_null = NULL, frames at stride
 * frame_len.  Variable-length frames: d_frame_off_or_null = n+1 offsets
 * (frame i = d_frames[off[i], off[i+1]), as rudp_encode_varlen writes them),
 * frame_len is a hint of the typical frame length (0 = unknown/tiny; it
 * picks lanes per frame, never the result) and the payload is zero-copy only
 * (d_payload_out_or_null must be NULL).  d_csum_in_or_null: rudp5 sideband checksums to verify
 * (NULL: d_ok = RUDP_OK_UNVERIFIED).  d_csum_out_or_null: the recomputed
 * checksum per packet.  d_payload_out_or_null: n*(frame_len-layout) bytes,
 * payloads copied out aligned; NULL = zero-copy (view at frame offset layout).
 * Frames shorter than the header get d_ok = RUDP_OK_SHORT and the fields
 * that are present (truncated as utils/packet.py:31 slices them), 0 otherwise.
 * Fixed-length frames whose payload is not a multiple of 16 bytes, or whose
 * buffers are not 16-byte aligned, decode through the variable-length tiles
 * with implicit offsets (a payload copy-out is one more launch), with the
 * same results; buffers are read as rudp_encode reads them.
 */
RUDP_API int rudp_decode(const uint8_t* d_frames, const uint64_t* d_frame_off_or_null,
                uint32_t frame_len, uint64_t n, const uint16_t* d_csum_in_or_null,
                uint16_t* d_seq, uint16_t* d_ack, uint8_t* d_flags, uint8_t* d_ok,
                uint16_t* d_csum_out_or_null, uint8_t* d_payload_out_or_null,
                int layout, int device, void* hip_stream);

/*
 * Frame + checksum a device-resident VARIABLE-LENGTH batch (in->len set).
 * The reference's own traffic: one UTF-8 character per datagram, 5-9 byte
 * frames (utils/reliableUDP.py:11, :53-61).  d_frame_off receives n+1
 * offsets, the exclusive scan of len[i] + layout (d_frame_off[n] = total
 * bytes); d_frames must hold sum(len) + n*layout bytes.  The concatenated
 * frames equal N calls of Packet(...).to_byte() back to back.
 */
RUDP_API int rudp_encode_varlen(const rudp_batch* in, uint8_t* d_frames, uint64_t* d_frame_off,
                       uint16_t* d_csum_or_null, int layout, int device, void* hip_stream);

/*
 * Sync-free forms of the two variable-length calls: the argument checks of
 * rudp_varlen_bounds / rudp_frame_off_bounds run on the device inside the call
 * (folded into the offset scan for encode; inside the decode kernels, where
 * every frame checks its own pair of offsets and a rejected frame gets
 * d_ok = RUDP_OK_BAD_OFFSETS) and land in *d_status (RUDP_ST_*), so the host
 * never waits.  The
 * caller reads d_status whenever it next synchronizes (the Python layer:
 * VarlenFrames.check() / DecodedBatch.check()).
 * rudp_encode_varlen_checked: payload_bytes = size of in->payload; frames_cap =
 *   capacity of d_frames.  Packed payloads (payload_off NULL) must satisfy
 *   sum(len) == payload_bytes; gathered ones payload_off[i] + len[i] <=
 *   payload_bytes.  d_frame_off[n] is always written; d_frame_off[0..n-1]
 *   when the batch is valid (status 0).
 * rudp_decode_varlen_checked: rudp_decode with offsets (zero-copy payload);
 *   frame_off[0..n] must be non-decreasing and <= frames_bytes.  d_status may
 *   be NULL (ABI 5): the call is then its one decode kernel, and the rejected
 *   frames are exactly those with d_ok == RUDP_OK_BAD_OFFSETS; with a status
 *   word the call zeroes it first (one more stream operation).
 * rudp_frame_off_check: only the offset check, for callers that run their own
 *   kernels on the frames afterwards.
 */
RUDP_API int rudp_encode_varlen_checked(const rudp_batch* in, uint64_t payload_bytes, uint8_t* d_frames,
                               uint64_t frames_cap, uint64_t* d_frame_off, uint16_t* d_csum_or_null,
                               uint32_t* d_status, int layout, int device, void* hip_stream);
RUDP_API int rudp_decode_varlen_checked(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                               uint32_t len_hint, uint64_t n, const uint16_t* d_csum_in_or_null,
                               uint16_t* d_seq, uint16_t* d_ack, uint8_t* d_flags, uint8_t* d_ok,
                               uint16_t* d_csum_out_or_null, uint32_t* d_status, int layout, int device,
                               void* hip_stream);
RUDP_API int rudp_frame_off_check(const uint64_t* d_frame_off, uint64_t n, uint64_t frames_bytes, uint32_t* d_status,
                         int device, void* hip_stream);

/*
 * Decode and strict-UTF-8 check in one pass (ABI 6): the reference's receive
 * parses every datagram AND decodes its payload (utils/reliableUDP.py:118-123:
 * Packet(data) -> get_header_field ... -> get_payload, whose strict
 * bytes.decode() is utils/packet.py:73).  As rudp_decode /
 * rudp_decode_varlen_checked, plus d_valid_or_null: d_valid[i] = 1 when
 * Packet(frame).get_payload() would return (an empty payload or a frame
 * shorter than the header: None), 0 when it would raise UnicodeDecodeError
 * -- rudp_validate_utf8's answer -- and 0 for a frame rejected for bad
 * offsets (nothing of it is read).  The LDS-tile decode kernels (fixed-length
 * frames whose 256/G-frame tile fits 64 KiB; packed frames of every hint)
 * judge each payload from the bytes they already hold, so every frame leaves
 * HBM once; other fixed-length shapes run the validation kernel after the
 * decode.  d_valid_or_null NULL: exactly rudp_decode / rudp_decode_varlen_checked.
 */
RUDP_API int rudp_decode_utf8(const uint8_t* d_frames, const uint64_t* d_frame_off_or_null, uint32_t frame_len,
                     uint64_t n, const uint16_t* d_csum_in_or_null, uint16_t* d_seq, uint16_t* d_ack,
                     uint8_t* d_flags, uint8_t* d_ok, uint16_t* d_csum_out_or_null,
                     uint8_t* d_payload_out_or_null, uint8_t* d_valid_or_null, int layout, int device,
                     void* hip_stream);
RUDP_API int rudp_decode_varlen_utf8(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                            uint32_t len_hint, uint64_t n, const uint16_t* d_csum_in_or_null,
                            uint16_t* d_seq, uint16_t* d_ack, uint8_t* d_flags, uint8_t* d_ok,
                            uint16_t* d_csum_out_or_null, uint8_t* d_valid_or_null, uint32_t* d_status,
                            int layout, int device, void* hip_stream);

/*
 * Packed payload copy-out of packed frames (ABI 8): the step the reference's
 * receive takes after parsing, `buffer + payload` for every accepted datagram
 * (utils/reliableUDP.py:121, :135-136) -- the message is the payloads of the
 * accepted frames back to back -- and the inverse of the packed
 * rudp_encode_varlen: what a relay that drops corrupt or retransmitted
 * datagrams and re-frames the rest (proxy.py:90-94) feeds the encode.
 * Sync-free as the *_checked calls: asynchronous on hip_stream, the host
 * never waits, temporaries come from the stream's set (usable under stream
 * capture), and *d_status (required) is written once per call, 0 when valid.
 * Per frame i < n (frames as rudp_decode_varlen_checked takes them):
 *   rejected  frame_off[i] > frame_off[i+1] or frame_off[i+1] > frames_bytes
 *             (the decode's per-frame rule, judged whether or not the frame
 *             is kept): plen[i] = 0, nothing of the frame is read, and
 *             RUDP_ST_OFFSETS is set;
 *   dropped   d_keep_or_null[i] == 0 (NULL: every frame kept): plen[i] = 0;
 *   kept      plen[i] = max(frame length - layout, 0): a frame shorter than
 *             the header contributes nothing.
 * d_payload_off[0..n] receives the exclusive scan of plen (d_payload_off[n] =
 * the total); all n + 1 entries are always written.  When the total exceeds
 * payload_cap, RUDP_ST_PAYLOAD_CAP is set and no byte of d_payload is written
 * (the caller reads the size it needs from d_payload_off[n]); otherwise
 * d_payload[payload_off[i], payload_off[i+1]) is frame i's payload, and
 * nothing is written outside [0, total) of d_payload: no byte before it and
 * none from `total` on, even inside payload_cap.  d_payload and
 * d_payload_off + a u32 len array of their differences are rudp_batch's
 * packed payload.  d_payload must not overlap d_frames: compaction in place
 * is not supported.  len_hint: the typical frame length (0 = unknown/tiny),
 * which picks the tile geometry, never the result; frames of any length the
 * buffer can hold are gathered.  n == 0 returns 0 and touches nothing.
 * Totals of 2^53 bytes and more (only overlapping frames can reach them)
 * are reported as RUDP_ST_PAYLOAD_CAP with d_payload_off unspecified.
 */
RUDP_API int rudp_gather_payloads(const uint8_t* d_frames, uint64_t frames_bytes,
                                  const uint64_t* d_frame_off, uint32_t len_hint, uint64_t n,
                                  const uint8_t* d_keep_or_null, uint8_t* d_payload,
                                  uint64_t payload_cap, uint64_t* d_payload_off,
                                  uint32_t* d_status, int layout, int device, void* hip_stream);

/*
 * A UTF-8 message cut into datagrams on the device (added within ABI 8,
 * RUDP_HAS_SEGMENT_UTF8): the sender's loop of utils/reliableUDP.py:44-60 --
 * slice k is message[k*PAYLOAD_SIZE : (k+1)*PAYLOAD_SIZE] in *characters*
 * (:44, :60), seq = ISN + character pointer (:54), ack 0 (:55), SYN on the
 * first frame (:45, :56-57) and FIN on the last (:46, :58-59); an empty
 * message is one SYN|FIN frame -- for any characters per datagram.  The
 * result is the header table and lengths of the packed rudp_batch whose
 * payload is d_msg itself (payload_off = NULL), as rudp_encode_varlen[_checked]
 * takes it.  The inverse of rudp_gather_payloads on the sending side.
 * Sync-free: asynchronous on hip_stream, the host never waits, temporaries
 * come from the stream's set.
 *
 * Characters and packets.  A byte b is a lead byte when (b & 0xC0) != 0x80;
 * `characters` is the number of lead bytes in d_msg[0, msg_bytes), which for
 * valid UTF-8 is Python's len(message).  Validity is not judged here
 * (rudp_validate_utf8 does that).  packets = max(1, ceil(characters /
 * chunk_chars)).  Packet 0 starts at byte 0, so continuation bytes before the
 * first lead byte belong to it; packet k >= 1 starts at the lead byte of
 * character k * chunk_chars; packet k ends where packet k + 1 starts and the
 * last one at msg_bytes.  A message without a lead byte, the empty one
 * included, is one packet holding all its bytes.
 *
 * Per packet k < packets:
 *   d_seq[k]   = (isn + k * chunk_chars) mod 2^16 (computed in 64 bits; isn is
 *                taken mod 2^16, as set_header_field keeps the low 16 bits,
 *                utils/packet.py:56)
 *   d_ack[k]   = 0
 *   d_flags[k] = 0x80 when k == 0, or'ed with 0x20 when k == packets - 1
 *   d_len[k]   = the packet's bytes
 *   d_payload_off_or_null[k] = the packet's first byte, and
 *                d_payload_off[packets] = msg_bytes (when not NULL)
 * d_count[0] = packets and d_count[1] = characters are always written.
 * *d_status is the call's status word, final when the call's work on the
 * stream is done, 0 when valid: RUDP_ST_PACKETS_CAP when packets >
 * max_packets; RUDP_ST_LEN when a packet exceeds 65535 bytes (only invalid
 * UTF-8 can: chunk_chars <= 16383 characters of at most 4 bytes).  With a
 * non-zero status only d_count is specified.  max_packets == 0 is the size
 * query: the table pointers may be NULL, d_count is written and the status is
 * RUDP_ST_PACKETS_CAP.  Nothing is ever written at index >= max_packets of
 * the tables nor at index > max_packets of d_payload_off; entries in
 * [packets, max_packets) are unspecified.
 *
 * RUDP_EINVAL, before any HIP call: chunk_chars outside [1, 16383]; d_count
 * or d_status NULL; d_msg NULL with msg_bytes > 0; d_seq, d_ack, d_flags or
 * d_len NULL with max_packets > 0.  An unaligned d_msg is read as unaligned
 * buffers are everywhere: whole aligned 16-byte blocks from the boundary at
 * or below its first byte to the one at or above its last.
 */
RUDP_API int rudp_segment_utf8(const uint8_t* d_msg, uint64_t msg_bytes, uint32_t chunk_chars,
                               uint32_t isn, uint64_t max_packets,
                               uint16_t* d_seq, uint16_t* d_ack, uint8_t* d_flags, uint32_t* d_len,
                               uint64_t* d_payload_off_or_null, uint64_t* d_count,
                               uint32_t* d_status, int device, void* hip_stream);

/*
 * The receiver's decision between decode and gather: which datagrams of a
 * batch it accepts (added within ABI 8, RUDP_HAS_ACCEPT_INORDER) --
 * receive_data of utils/reliableUDP.py:116-137, stop-and-wait: a SYN opens a
 * transfer (:128-132), then only the frame whose seq_num equals ISN +
 * characters received so far is accepted (:124, :134-136) -- and the ack_num
 * of the reply send_ack builds for every datagram (:139-146).  Both calls are
 * sync-free: asynchronous on hip_stream, the host never waits, usable under
 * stream capture.
 *
 * The rule, in absolute sequence space.  The state is expect = ISN +
 * characters received (an integer that is never reduced mod 2^16), isn, and
 * live (the receiver has a peer, self.target_addr).  last_isn is the previous
 * transfer's ISN (self.prev_random_number), constant during one recv(); a
 * value above 65535 means none.  Per frame i in arrival order, with seq_i,
 * syn_i = flags & 0x80, fin_i = flags & 0x20, c_i the characters of its
 * payload and usable_i:
 *   ignored    !usable_i: nothing changes, no reply.  syn_i && seq_i ==
 *              last_isn (a repeated SYN, :126): nothing changes, but a reply
 *              is sent.
 *   reset      syn_i otherwise: isn = seq_i, expect = seq_i + c_i, live = 1;
 *              the frame is accepted and the message restarts at this frame.
 *   in-order   a non-SYN with live && seq_i == expect, compared as integers
 *              (once expect > 65535 nothing matches, as in the reference):
 *              the frame is accepted and expect += c_i.
 *   else       not accepted.
 * A reply is sent for every usable frame while live is set after the frame;
 * its ack_num is expect after the frame, mod 2^16.  The first accepted frame
 * with FIN ends the call's transfer at index `end`; frames after `end` belong
 * to the next recv() and are not judged.  With live == 0 nothing before the
 * first reset is accepted or answered (the reference clears its buffer and
 * sends nothing while target_addr is None, :140-141).
 *
 * rudp_payload_chars: d_chars[i] = c_i, the number of lead bytes
 * ((b & 0xC0) != 0x80, rudp_segment_utf8's definition; Python's len() for
 * valid UTF-8) of frame i from byte `layout` on.  Packed frames with n + 1
 * offsets, frames_bytes and len_hint as rudp_gather_payloads takes them: a
 * frame shorter than the header gives 0; a frame whose pair of offsets is
 * decreasing or past frames_bytes gives 0 and none of its bytes is read.
 * len_hint picks the lanes per frame, never the result; frames of any length
 * the buffer holds are counted (mod 2^32).  An unaligned d_frames is read as
 * whole aligned 16-byte blocks, as everywhere.  n == 0 returns 0 and touches
 * nothing.  RUDP_EINVAL before any HIP call: a layout other than 5 or 7;
 * with n > 0, d_frame_off or d_chars NULL, or d_frames NULL with frames_bytes.
 *
 * rudp_accept_inorder: d_seq, d_flags as the decode wrote them, d_chars from
 * rudp_payload_chars, d_usable_or_null[i] != 0 for a usable frame (NULL: all
 * usable), d_state_in = {expect, isn, live, 0}.  Outputs, n entries each:
 *   d_accept[i]    1 when frame i is accepted by the rule
 *   d_keep[i]      1 when it is accepted, at or after the last reset at or
 *                  before `end`, and at or before `end`: the keep mask of
 *                  rudp_gather_payloads for this call's part of the message
 *   d_reply[i]     1 when a reply is sent for it, d_reply_ack[i] its ack_num
 *                  (0 where d_reply[i] is 0)
 * and all four are 0 for i > end.  d_state_out (u64[4], may be d_state_in):
 * the state after frame `end`, or after all n.  d_info (u64[6]):
 *   [0] end (n when no accepted frame has FIN)
 *   [1] the number of accepted frames
 *   [2] msg_start: the index of the last reset at or before `end` (n when
 *       there is none: the caller's carried buffer continues)
 *   [3] the message's characters so far, expect - isn when live, else 0
 *   [4] first_anomaly: the index where the one-scan form stopped being exact
 *       and the sequential form took over (n when it never did; see DESIGN)
 *   [5] 0, reserved
 * n == 0 copies the state, writes d_info = {0, 0, 0, characters, 0, 0} and
 * nothing else.  Temporaries come from the stream's set.  RUDP_EINVAL before
 * any HIP call: d_state_in, d_state_out or d_info NULL; with n > 0, d_seq,
 * d_flags, d_chars, d_accept, d_keep, d_reply or d_reply_ack NULL.
 */
RUDP_API int rudp_payload_chars(const uint8_t* d_frames, uint64_t frames_bytes,
                                const uint64_t* d_frame_off, uint32_t len_hint, uint64_t n,
                                uint32_t* d_chars, int layout, int device, void* hip_stream);
RUDP_API int rudp_accept_inorder(const uint16_t* d_seq, const uint8_t* d_flags, const uint32_t* d_chars,
                                 const uint8_t* d_usable_or_null, uint64_t n, uint32_t last_isn,
                                 const uint64_t* d_state_in, uint8_t* d_accept, uint8_t* d_keep,
                                 uint8_t* d_reply, uint16_t* d_reply_ack, uint64_t* d_state_out,
                                 uint64_t* d_info, int device, void* hip_stream);

/*
 * The reordering receiver of a windowed sender (added within ABI 8,
 * RUDP_HAS_ACCEPT_WINDOW): rudp_accept_inorder's rule with a pending set, for
 * the sender that keeps several frames in flight and takes cumulative replies
 * (RUDP_ACK_CUMULATIVE).  Defined by this library (the reference never has
 * two frames in flight); with window_chars == 1 nothing can be ahead inside
 * the window and the rule is rudp_accept_inorder's.  Both calls are sync-free:
 * asynchronous on hip_stream, the host never waits, temporaries come from the
 * stream's set, usable under stream capture.
 *
 * rudp_accept_window.  d_seq, d_flags, d_chars, d_usable_or_null, n, last_isn
 * and d_state_in = {expect, isn, live, 0} as rudp_accept_inorder takes them;
 * window_chars (Wc) in [1, 1024]; n_carried <= min(n, 1023): the first
 * n_carried frames are the ones the call before left pending, presented again
 * in the order that call gave them.  They are judged as every other frame and
 * get no reply.  The pending set is not part of the state (u64[4],
 * interchangeable with rudp_accept_inorder's): it is empty on entry.
 *
 * The rule, per frame i in arrival order; P maps a start to a pending frame:
 *   ignored    !usable_i, or syn_i && seq_i == last_isn (a reply is sent for
 *              the latter), as rudp_accept_inorder.
 *   reset      syn_i otherwise: isn = seq_i, expect = seq_i + c_i, live = 1;
 *              the frames in P are rejected and P is emptied; the delivery
 *              order restarts with this frame at rank 0 (frames delivered
 *              before it keep accept = 1 and lose their rank); with fin_i the
 *              transfer ends here.
 *   in-order   a non-SYN with live && seq_i == expect (as integers): delivered,
 *              expect += c_i; with fin_i the transfer ends here; otherwise,
 *              while P holds a frame that starts at expect, that frame is
 *              delivered next, its c added and the frame removed, and the
 *              transfer ends with the first such frame that has FIN.  Then
 *              every frame of P that starts below expect is rejected.
 *   ahead      a non-SYN with live, expect < seq_i < expect + Wc, c_i > 0 and
 *              no frame of P with the same start: pending (its FIN counts
 *              when it is delivered).
 *   else       rejected: a past frame, one at or beyond the window, c_i == 0
 *              ahead of expect, a second frame for a pending start.
 * A reply is sent for every usable frame i >= n_carried while live is set
 * after it; its ack_num is expect after the frame (after the drain) mod 2^16:
 * a cumulative acknowledgement.  `end` is the arrival index of the frame whose
 * step delivered a FIN; P is emptied then, and the frames after `end` are not
 * judged (every output 0, ranks RUDP_RANK_NONE).  Once expect > 65535 nothing
 * matches.  Outputs, n entries each:
 *   d_accept[i]     1: delivered at some point of the call; 2: pending when
 *                   the call ends; 0 otherwise
 *   d_rank[i]       u32: a delivered frame's position in this call's part of
 *                   the message, in delivery order counted from the last
 *                   reset at or before `end` (from the first delivery when
 *                   there is none); else RUDP_RANK_NONE
 *   d_carry_rank[i] u32: a pending frame's position among the pending ones,
 *                   in arrival order; else RUDP_RANK_NONE
 *   d_reply[i], d_reply_ack[i]   as rudp_accept_inorder
 * d_state_out (u64[4], may be d_state_in); d_info (u64[8]): [0] end (n: no
 * FIN was delivered) [1] K, the ranked frames [2] msg_start (the last reset at
 * or before `end`, n: none) [3] characters so far [4] first_anomaly: the first
 * frame a chunk of the device form gave to its sequential walk (n: none; see
 * DESIGN) [5] frames pending at the end [6] frames ever delivered [7] 0.
 * n == 0 copies the state and writes d_info = {0, 0, 0, characters, 0, 0, 0,
 * 0}.  RUDP_EINVAL before any HIP call: d_state_in, d_state_out or d_info
 * NULL; window_chars outside [1, 1024]; n_carried above min(n, 1023); n above
 * 2^32 - 2; with n > 0, d_seq, d_flags, d_chars, d_accept, d_rank,
 * d_carry_rank, d_reply or d_reply_ack NULL.
 *
 * rudp_gather_ordered: rudp_gather_payloads with a permutation.  Frames,
 * frames_bytes, d_frame_off[n + 1], len_hint and n as the gather takes them;
 * d_rank u32[n]; d_count, a device u64: the K the ranks run to, read on the
 * device (K above n counts as n); skip in {0, 5, 7}: the bytes left out at the
 * head of every frame.  Frame i with d_rank[i] = r < K writes max(len_i -
 * skip, 0) bytes at d_out_off[r], the exclusive scan of those lengths in rank
 * order: d_out_off[0..K] are written (d_out_off[K] the total) and, when not
 * NULL, d_src_or_null[k] = the frame with rank k for k < K (RUDP_RANK_NONE
 * when no frame has it).  With d_rank/d_info[1] and skip = layout this is the
 * message of rudp_accept_window; with d_carry_rank/d_info[5] and skip 0, its
 * pending frames whole, for the next call.  *d_status (required): 0, or
 * RUDP_ST_OFFSETS when a ranked frame's offsets are decreasing or past
 * frames_bytes (it contributes 0 bytes and is not read), RUDP_ST_RANK when a
 * rank at or above K is not RUDP_RANK_NONE (the frame is skipped),
 * RUDP_ST_PAYLOAD_CAP when the total exceeds out_cap (no byte of d_out is
 * written; d_out_off[K] holds the size needed).  Nothing is written at or past
 * the total of d_out, nor past index K of d_out_off or K - 1 of d_src.  d_out
 * must not overlap d_frames.  The ranks below K must be distinct; when they
 * are not the result is unspecified and every access stays in bounds.  n == 0
 * returns 0 and touches nothing.  RUDP_EINVAL before any HIP call: skip not 0,
 * 5 or 7; d_status or d_count NULL; n above 2^32 - 2; with n > 0, d_frame_off,
 * d_rank or d_out_off NULL, d_frames NULL with frames_bytes > 0, d_out NULL
 * with out_cap > 0.
 */
#define RUDP_RANK_NONE 0xFFFFFFFFu
RUDP_API int rudp_accept_window(const uint16_t* d_seq, const uint8_t* d_flags, const uint32_t* d_chars,
                                const uint8_t* d_usable_or_null, uint64_t n, uint32_t last_isn,
                                uint32_t window_chars, uint64_t n_carried, const uint64_t* d_state_in,
                                uint8_t* d_accept, uint32_t* d_rank, uint32_t* d_carry_rank, uint8_t* d_reply,
                                uint16_t* d_reply_ack, uint64_t* d_state_out, uint64_t* d_info, int device,
                                void* hip_stream);
RUDP_API int rudp_gather_ordered(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                                 uint32_t len_hint, uint64_t n, const uint32_t* d_rank, const uint64_t* d_count,
                                 uint32_t skip, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_off,
                                 uint32_t* d_src_or_null, uint32_t* d_status, int device, void* hip_stream);

/*
 * One datagram batch judged for many peers (added within ABI 8,
 * RUDP_HAS_ACCEPT_FLOWS): a server's recvmmsg batch carries datagrams of many
 * concurrent transfers; every transfer is judged by rudp_accept_inorder's
 * rule, independently, in one launch, with all per-peer state in a device
 * table.  Sync-free: asynchronous on hip_stream, the host never waits, no
 * temporaries, usable under stream capture.
 *
 * d_seq, d_flags, d_chars, d_usable_or_null and n as rudp_accept_inorder takes
 * them; d_flow[i] (u32) is the slot of datagram i's peer.  d_states is
 * u64[n_flows][4], read and written in place; a row is {expect, isn, live,
 * last_isn + 1}, word 3 == 0 meaning "no previous transfer", so an all-zero
 * table is a table of fresh flows.  Only the rows of slots that occur in the
 * batch are read or written; the call does no work proportional to n_flows.
 *
 * Per flow the rule is exactly rudp_accept_inorder's, applied to the flow's
 * datagrams in arrival order with the row as d_state_in and word 3 - 1 as
 * last_isn (none when word 3 is 0 or above 65536).  A datagram with d_flow[i]
 * == RUDP_FLOW_NONE is ignored as an unusable one is; one with d_flow[i] >=
 * n_flows is ignored too and sets RUDP_ST_FLOW.  An ignored datagram gets
 * every output 0, rank RUDP_RANK_NONE, and touches no row.
 *
 * The flow's first accepted FIN ends that flow's transfer (arrival index
 * end_f): its later datagrams in this call are not judged (outputs 0), and
 * the flow turns over on the device, its row becomes {0, 0, 0, isn + 1}: a
 * closed flow that accepts and answers nothing until a SYN arrives whose seq
 * differs from that ISN.  (live = 0 after the end is this library's choice;
 * the single-peer receiver keeps answering its old peer.)  A flow that does
 * not end gets {expect, isn, live, word 3 unchanged}.
 *
 * Per-datagram outputs, n entries each, in arrival order: d_accept, d_keep,
 * d_reply, d_reply_ack as rudp_accept_inorder defines them, per flow (keep:
 * accepted, at or after the flow's last reset at or before its end, and at or
 * before its end); d_rank[i] (u32): a kept datagram's position in the
 * flow-major message order (ascending slot, arrival order within a slot),
 * else RUDP_RANK_NONE.  With d_rank, d_info + 1 as d_count and skip = layout,
 * rudp_gather_ordered writes all flows' message pieces back to back.
 *
 * Grouping outputs, A = the distinct valid slots of the batch:
 *   d_order[n]        u32: the arrival indices, flow-major; the datagrams
 *                     without a valid slot follow, in arrival order
 *   d_order_off[0..A] u32: where each active flow's run starts in d_order;
 *                     [A]: where the flowless ones start (provide n + 1)
 *   d_flow_info       u64[A][8], ascending by slot (provide n rows): [0] slot
 *                     [1] end (arrival index; n: none) [2] accepted datagrams
 *                     [3] msg_start (arrival index of the last reset at or
 *                     before the end; n: none) [4] characters so far (expect -
 *                     isn when live, else 0; before the turn-over) [5] isn
 *                     (before the turn-over) [6] kept datagrams [7] rank base
 *                     (the kept datagrams of the flows before it)
 *   d_info            u64[8]: [0] A [1] K, the kept total [2] R, the replies
 *                     [3] flows that ended [4] datagrams without a valid slot
 *                     [5] flows the kernel judged sequentially (a diagnostic,
 *                     not part of the contract) [6..7] 0
 *   *d_status         required: 0 or RUDP_ST_FLOW
 * Nothing is written past index A of d_order_off or past row A - 1 of
 * d_flow_info.  n == 0 writes d_info = 0 and *d_status = 0 and touches nothing
 * else.  n > RUDP_FLOWS_MAX_BATCH returns RUDP_ENOTSUP (a recvmmsg batch never
 * exceeds it).  RUDP_EINVAL before any HIP call: d_states, d_info or d_status
 * NULL; n_flows 0 or above 2^32 - 2; with n > 0, any other pointer except
 * d_usable_or_null NULL.
 */
#define RUDP_HAS_ACCEPT_FLOWS 1
#define RUDP_FLOW_NONE 0xFFFFFFFFu
#define RUDP_FLOWS_MAX_BATCH 1024u
#define RUDP_ST_FLOW 256u   /* a d_flow[i] at or above n_flows that is not RUDP_FLOW_NONE */
RUDP_API int rudp_accept_flows(const uint16_t* d_seq, const uint8_t* d_flags, const uint32_t* d_chars,
                               const uint8_t* d_usable_or_null, const uint32_t* d_flow, uint64_t n,
                               uint64_t* d_states, uint64_t n_flows,
                               uint8_t* d_accept, uint8_t* d_keep, uint8_t* d_reply, uint16_t* d_reply_ack,
                               uint32_t* d_rank, uint32_t* d_order, uint32_t* d_order_off,
                               uint64_t* d_flow_info, uint64_t* d_info, uint32_t* d_status,
                               int device, void* hip_stream);

/*
 * A datagram batch to message and replies in one call (added within ABI 8,
 * RUDP_HAS_RECEIVE): what the reference's recv() loop makes of the datagrams
 * of one recvmmsg (utils/reliableUDP.py:97-137) and the send_ack packets it
 * answers them with (:139-146).  One call does rudp_decode_varlen_utf8, the
 * usable mask, rudp_payload_chars, rudp_accept_inorder and
 * rudp_gather_payloads (keep as the mask), every output bit for bit what
 * those calls write, and builds the reply datagrams.  Sync-free as the
 * *_checked calls: asynchronous on hip_stream, the host never waits,
 * temporaries come from the stream's set, usable under stream capture.  A
 * batch of at most 1024 datagrams in at most 32768 bytes and 261 bytes per
 * datagram (a recvmmsg batch of this protocol) is one launch of one workgroup
 * that reads the frames once;
 * larger batches run the launches of the five calls and a reply builder.
 *
 * Inputs: d_frames, frames_bytes, d_frame_off[n + 1], len_hint, n,
 * d_csum_in_or_null and layout as rudp_decode_varlen_utf8 takes them;
 * last_isn and d_state_in[4] as rudp_accept_inorder.  Outputs through *out
 * (device pointers; n entries each unless said otherwise):
 *   seq, ack, flags, ok, csum_out_or_null, valid
 *                 as rudp_decode_varlen_utf8 writes them
 *   usable        u8: 1 when ok is RUDP_OK_GOOD or RUDP_OK_UNVERIFIED and
 *                 valid == 1.  (RUDP_OK_UNVERIFIED occurs only for layout 5
 *                 without a sideband checksum, and then for every frame that
 *                 is long enough.)  A short frame, a frame with a wrong
 *                 checksum or invalid UTF-8, and a frame with bad offsets
 *                 (RUDP_OK_BAD_OFFSETS) are not usable.
 *   chars         u32: rudp_payload_chars' answer
 *   accept, keep, reply, reply_ack, state_out[4] (may be d_state_in)
 *                 as rudp_accept_inorder, with `usable` as its mask
 *   payload, payload_cap, payload_off[n + 1]
 *                 as rudp_gather_payloads with `keep` as its mask: when the
 *                 total exceeds payload_cap, RUDP_ST_PAYLOAD_CAP is set, no
 *                 byte of payload is written and payload_off[n] holds the size
 *                 needed; nothing is ever written at or past the total
 *   reply_frames  with R = the number of i with reply[i] == 1: R header-only
 *                 frames of `layout` bytes at stride `layout`, in arrival
 *                 order, the k-th being Packet().to_byte() of seq 0, ack =
 *                 reply_ack[i], flags 0x40 (for layout 7 with the RFC 1071
 *                 checksum of the header in-band).  The caller provides
 *                 n * layout bytes; nothing is written at or past R * layout.
 *   reply_csum_or_null  u16[R]: the checksum of each reply frame (the layout 5
 *                 sideband; for layout 7 a copy of the in-band value)
 *   reply_index   u32[R]: the datagram index i of reply k
 *   reply_peer    u64[R]: the index of the last reset (rudp_accept_inorder's
 *                 rule) at or before datagram i, or n when this batch has none
 *                 before it: the datagram whose source address the reply goes
 *                 to (self.target_addr, :131, :146); n is the peer carried
 *                 from earlier batches
 *   info          u64[8]: [0..4] as rudp_accept_inorder's d_info; [5] = R;
 *                 [6] = the message bytes of this batch (payload_off[n]);
 *                 [7] = 0, reserved
 *   status        u32, required: final when the call's work on the stream is
 *                 done, 0 when valid; RUDP_ST_OFFSETS when any frame was
 *                 rejected for its offsets, RUDP_ST_PAYLOAD_CAP as above
 * n == 0 copies the state, writes info (as rudp_accept_inorder's n == 0, with
 * [5] = [6] = 0) and status = 0, and touches nothing else.
 * RUDP_EINVAL before any HIP call: out NULL; a layout other than 5 or 7; a
 * sideband d_csum_in with layout 7; d_state_in, state_out, info or status
 * NULL; n above 2^32 - 1; with n > 0, d_frame_off or any table other than
 * csum_out_or_null and reply_csum_or_null NULL, d_frames NULL with
 * frames_bytes > 0, or payload NULL with payload_cap > 0.
 */
#define RUDP_HAS_RECEIVE 1
typedef struct rudp_received {
  uint16_t* seq;
  uint16_t* ack;
  uint8_t* flags;
  uint8_t* ok;
  uint16_t* csum_out_or_null;
  uint8_t* valid;
  uint8_t* usable;
  uint32_t* chars;
  uint8_t* accept;
  uint8_t* keep;
  uint8_t* reply;
  uint16_t* reply_ack;
  uint64_t* state_out;
  uint8_t* payload;
  uint64_t payload_cap;
  uint64_t* payload_off;
  uint8_t* reply_frames;
  uint16_t* reply_csum_or_null;
  uint32_t* reply_index;
  uint64_t* reply_peer;
  uint64_t* info;
  uint32_t* status;
} rudp_received;
RUDP_API int rudp_receive(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                          uint32_t len_hint, uint64_t n, const uint16_t* d_csum_in_or_null, uint32_t last_isn,
                          const uint64_t* d_state_in, const rudp_received* out, int layout, int device,
                          void* hip_stream);

/*
 * The reordering receiver in one call (added within ABI 8,
 * RUDP_HAS_RECEIVE_WINDOW): rudp_receive for a windowed sender.  One call
 * does rudp_decode_varlen_utf8, the usable mask and rudp_payload_chars over
 * the frames the call before left pending followed by the new datagrams,
 * rudp_accept_window, rudp_gather_ordered twice (the message in delivery
 * order, the frames still pending whole) and builds the reply datagrams, every
 * output bit for bit what those calls write.  Sync-free as rudp_receive:
 * asynchronous on hip_stream, the host never waits, temporaries come from the
 * stream's set, usable under stream capture.  At most 1024 new datagrams with
 * at most 32768 bytes in both buffers and 1005 bytes per frame (a recvmmsg
 * batch of this protocol) are one launch of one workgroup that reads the
 * frames once; larger batches join the two buffers in a temporary and run the
 * launches of the calls above and a reply builder.
 *
 * Inputs.  The two sources stay separate buffers, each with its own offsets
 * and its own bound: carried item k is d_carried[co[k], co[k + 1]) with co =
 * d_carried_off[n_carried + 1], judged by the decode's per-frame offset rule
 * against carried_bytes; new item j is d_frames[fo[j], fo[j + 1]) with fo =
 * d_frame_off[n_new + 1], judged against frames_bytes.  n = n_carried + n_new;
 * item i < n_carried is carried frame i, else new frame i - n_carried.
 * len_hint and layout as rudp_decode_varlen_utf8; last_isn, window_chars,
 * n_carried and d_state_in[4] as rudp_accept_window.  Sideband checksums
 * (layout 5): item i < n_carried verifies against d_carried_csum_or_null[i],
 * the others against d_csum_in_or_null[i - n_carried]; with n_carried > 0 the
 * two are both given or both NULL, and both NULL with layout 7.
 *
 * A frame rejected by the offset rule gets ok = RUDP_OK_BAD_OFFSETS, valid =
 * usable = chars = 0 and header fields 0; none of its bytes is read,
 * RUDP_ST_OFFSETS is set, and it is never ranked and never pending.
 *
 * Outputs through *out (device pointers; n entries each unless said otherwise):
 *   seq, ack, flags, ok, csum_out_or_null, valid
 *                 as rudp_decode_varlen_utf8 writes them
 *   usable        as rudp_receive defines it
 *   chars         as rudp_payload_chars
 *   accept, rank, carry_rank, reply, reply_ack, state_out[4] (may be
 *   d_state_in), info[0..7]
 *                 exactly rudp_accept_window over the n items with `usable`
 *                 as its mask
 *   payload, payload_cap, payload_off[n + 1], payload_src_or_null[n]
 *                 the message: exactly rudp_gather_ordered(rank, K = info[1],
 *                 skip = layout); payload_off[0..K] and payload_src[0..K - 1]
 *                 are written.  When the total exceeds payload_cap,
 *                 RUDP_ST_PAYLOAD_CAP is set, no byte of payload is written
 *                 and payload_off[K] holds the size needed; nothing is written
 *                 at or past the total, nor past index K of payload_off
 *   carry_frames, carry_cap, carry_off[1024]
 *                 the frames still pending, whole: exactly
 *                 rudp_gather_ordered(carry_rank, P = info[5], skip = 0);
 *                 carry_off[0..P] are written; the overflow bit is
 *                 RUDP_ST_CARRY_CAP.  carry_frames must not overlap either
 *                 input buffer: callers ping-pong two sets
 *   carry_csum_or_null  u16[1023]: [k] = the input sideband checksum of the
 *                 frame with carry rank k, written only when the input
 *                 sidebands are given.  carry_frames, carry_off, carry_csum,
 *                 info[5] and info[10] are the next call's d_carried,
 *                 d_carried_off, d_carried_csum, n_carried and carried_bytes
 *   reply_frames, reply_csum_or_null, reply_index
 *                 as rudp_receive: R header-only frames of `layout` bytes in
 *                 arrival order (seq 0, ack = reply_ack[i], flags 0x40, the
 *                 checksum in-band for layout 7); reply_index[k] = i, always
 *                 >= n_carried (carried frames get no reply).  The caller
 *                 provides n_new * layout bytes (and n_new entries of the
 *                 tables); nothing is written at or past R * layout
 *   reply_peer    u64[R]: the index of the last reset (rudp_accept_inorder's
 *                 class) at an item in [n_carried, i], or n when there is none
 *   info          u64[12]: [8] = R; [9] = the message bytes (payload_off[K]);
 *                 [10] = the carried bytes (carry_off[P]); [11] = 0
 *   status        u32, required, written once: RUDP_ST_OFFSETS |
 *                 RUDP_ST_PAYLOAD_CAP | RUDP_ST_CARRY_CAP, or 0
 * n == 0 copies the state, writes info = {0, 0, 0, characters, 0, ... 0},
 * status = 0 and carry_off[0] = 0, and touches nothing else.
 * RUDP_EINVAL before any HIP call: out NULL; a layout other than 5 or 7; a
 * sideband with layout 7, or with n_carried > 0 only one of the two given;
 * window_chars outside [1, 1024]; n_carried > 1023; n above 2^32 - 2;
 * d_state_in, state_out, info or status NULL; with n > 0, any table other than
 * the _or_null ones NULL (reply_frames, reply_index and reply_peer only with
 * n_new > 0); d_frame_off NULL with n_new > 0; d_carried_off NULL with
 * n_carried > 0; a frames pointer NULL with its byte count > 0; payload NULL
 * with payload_cap > 0; carry_frames NULL with carry_cap > 0.
 */
#define RUDP_HAS_RECEIVE_WINDOW 1
typedef struct rudp_received_window {
  uint16_t* seq;
  uint16_t* ack;
  uint8_t* flags;
  uint8_t* ok;
  uint16_t* csum_out_or_null;
  uint8_t* valid;
  uint8_t* usable;
  uint32_t* chars;
  uint8_t* accept;
  uint32_t* rank;
  uint32_t* carry_rank;
  uint8_t* reply;
  uint16_t* reply_ack;
  uint64_t* state_out;
  uint8_t* payload;
  uint64_t payload_cap;
  uint64_t* payload_off;
  uint32_t* payload_src_or_null;
  uint8_t* carry_frames;
  uint64_t carry_cap;
  uint64_t* carry_off;
  uint16_t* carry_csum_or_null;
  uint8_t* reply_frames;
  uint16_t* reply_csum_or_null;
  uint32_t* reply_index;
  uint64_t* reply_peer;
  uint64_t* info;
  uint32_t* status;
} rudp_received_window;
RUDP_API int rudp_receive_window(const uint8_t* d_carried, uint64_t carried_bytes, const uint64_t* d_carried_off,
                                 const uint16_t* d_carried_csum_or_null, uint64_t n_carried,
                                 const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                                 const uint16_t* d_csum_in_or_null, uint64_t n_new, uint32_t len_hint,
                                 uint32_t last_isn, uint32_t window_chars, const uint64_t* d_state_in,
                                 const rudp_received_window* out, int layout, int device, void* hip_stream);

/*
 * The many-peer receiver in one call (added within ABI 8,
 * RUDP_HAS_RECEIVE_FLOWS): rudp_receive for a server whose recvmmsg batch
 * carries datagrams of many transfers.  One call does
 * rudp_decode_varlen_utf8, the usable mask, rudp_payload_chars,
 * rudp_accept_flows (usable as its mask) and rudp_gather_ordered(rank, K =
 * info[1], skip = layout), every output bit for bit what those calls write,
 * and builds the reply datagrams and, for every flow whose transfer ended, the
 * closing datagram its peer is owed.  Sync-free as rudp_receive: asynchronous
 * on hip_stream, the host never waits, temporaries come from the stream's
 * set, usable under stream capture.  A batch in at most 32768 bytes and 133
 * bytes per datagram is one launch of one workgroup that reads the frames
 * once; other batches run the launches of the five calls and one finishing
 * pass.
 *
 * Inputs: d_frames, frames_bytes, d_frame_off[n + 1], len_hint, n,
 * d_csum_in_or_null and layout as rudp_decode_varlen_utf8 takes them; d_flow,
 * d_states (read and written in place) and n_flows as rudp_accept_flows.  A
 * frame rejected by the offset rule gets ok = RUDP_OK_BAD_OFFSETS, is
 * unusable, sets RUDP_ST_OFFSETS and is never ranked.  Outputs through *out
 * (device pointers; n entries each unless said otherwise):
 *   seq, ack, flags, ok, csum_out_or_null, valid, usable, chars
 *                 as rudp_receive defines them
 *   accept, keep, reply, reply_ack, rank, order, order_off[n + 1],
 *   flow_info[n][8], info[0..7] and d_states
 *                 exactly rudp_accept_flows with `usable` as its mask
 *   payload, payload_cap, payload_off[n + 1], payload_src_or_null[n]
 *                 every active flow's message piece back to back in flow
 *                 order: exactly rudp_gather_ordered's; payload_off[0..K] and
 *                 payload_src[0..K - 1] are written (flow a's piece is
 *                 payload[payload_off[b], payload_off[b + kept]) with b =
 *                 flow_info[a][7], kept = flow_info[a][6]).  When the total
 *                 exceeds payload_cap, RUDP_ST_PAYLOAD_CAP is set, no byte of
 *                 payload is written and payload_off[K] holds the size needed;
 *                 nothing is written at or past the total
 *   reply_frames, reply_csum_or_null, reply_index
 *                 as rudp_receive: R = info[2] header-only frames of `layout`
 *                 bytes at stride `layout`, in arrival order (seq 0, ack =
 *                 reply_ack[i], flags 0x40, the checksum in-band for layout
 *                 7); reply_index[k] = i.  A reply goes to the source of its
 *                 own datagram, so there is no reply_peer.  The caller
 *                 provides n * layout bytes (and n entries of the tables);
 *                 nothing is written at or past R * layout
 *   fin_frames, fin_csum_or_null, fin_flow
 *                 E = info[3] closing datagrams, one for every active flow a
 *                 with flow_info[a][1] < n, in ascending a: the header-only
 *                 frame with seq 0, ack = (flow_info[a][5] + flow_info[a][4])
 *                 mod 2^16 (the ISN plus the characters received) and flags
 *                 0x60 (FIN|ACK), the checksum in-band for layout 7 and in
 *                 fin_csum for both layouts; fin_flow[e] = a (u32), the peer
 *                 being that of slot flow_info[a][0].  The caller provides
 *                 n * layout bytes and n entries; nothing is written at or
 *                 past E * layout
 *   info          u64[12]: [0..7] as rudp_accept_flows' d_info; [8] = the
 *                 message bytes (payload_off[K]); [9..11] = 0
 *   status        u32, required, written once: RUDP_ST_OFFSETS | RUDP_ST_FLOW
 *                 | RUDP_ST_PAYLOAD_CAP, or 0
 * n == 0 writes info = 0 and status = 0 and touches nothing else, not even
 * d_states.  n > RUDP_FLOWS_MAX_BATCH returns RUDP_ENOTSUP.  RUDP_EINVAL
 * before any HIP call: out NULL; a layout other than 5 or 7; a sideband
 * d_csum_in with layout 7; d_states, info or status NULL; n_flows 0 or above
 * 2^32 - 2; with n > 0, d_frame_off, d_flow or any table other than the
 * _or_null ones NULL, d_frames NULL with frames_bytes > 0, or payload NULL
 * with payload_cap > 0.
 */
#define RUDP_HAS_RECEIVE_FLOWS 1
typedef struct rudp_received_flows {
  uint16_t* seq;
  uint16_t* ack;
  uint8_t* flags;
  uint8_t* ok;
  uint16_t* csum_out_or_null;
  uint8_t* valid;
  uint8_t* usable;
  uint32_t* chars;
  uint8_t* accept;
  uint8_t* keep;
  uint8_t* reply;
  uint16_t* reply_ack;
  uint32_t* rank;
  uint32_t* order;
  uint32_t* order_off;
  uint64_t* flow_info;
  uint8_t* payload;
  uint64_t payload_cap;
  uint64_t* payload_off;
  uint32_t* payload_src_or_null;
  uint8_t* reply_frames;
  uint16_t* reply_csum_or_null;
  uint32_t* reply_index;
  uint8_t* fin_frames;
  uint16_t* fin_csum_or_null;
  uint32_t* fin_flow;
  uint64_t* info;
  uint32_t* status;
} rudp_received_flows;
RUDP_API int rudp_receive_flows(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                                uint32_t len_hint, uint64_t n, const uint16_t* d_csum_in_or_null,
                                const uint32_t* d_flow, uint64_t* d_states, uint64_t n_flows,
                                const rudp_received_flows* out, int layout, int device, void* hip_stream);

/*
 * The sender's judgement of a reply batch (added within ABI 8,
 * RUDP_HAS_ACKNOWLEDGE): wait_ack of utils/reliableUDP.py:64-85 for every
 * reply datagram of one recvmmsg, and the closing packet of send_ack (:87-93).
 * Both calls are sync-free: asynchronous on hip_stream, the host never waits,
 * temporaries come from the stream's set, usable under stream capture.
 *
 * The rule.  Constants of one send(): isn (self.random_number, at most 65535),
 * T = total_chars (len(message)), C = chunk_chars (PAYLOAD_SIZE).  State, u64[4]
 * {p, L, last, done}: p characters acknowledged (self.message_pointer), L the
 * characters of the outstanding frame (payload_length), last != 0 when that
 * frame is the message's last (is_last), done.  A fresh transfer starts at
 * p = 0, L = min(C, T), last = (L == T), done = 0.  Per reply i in arrival
 * order, with seq_i, ack_i, flags_i and usable_i:
 *   expected = isn + p + L, an integer that is never reduced mod 2^16;
 *   valid_i  = usable_i && ack_i == expected (RUDP_ACK_EXACT, :71; once
 *              expected > 65535 nothing matches, as in the reference);
 *   !valid_i: nothing changes (:75-76).  Otherwise:
 *   flags_i & 0x40 (ACK): p = ack_i - isn (:77-78);
 *   flags_i & 0x20 (FIN): end = i, done = 1, and the call's judging stops; the
 *              closing datagram has seq = (isn + p) mod 2^16, ack = (seq_i + 1)
 *              mod 2^16 and flags 0x40 (:79-80, :87-93);
 *   else last: L = 0 (everything is sent: wait for the FIN at isn + p, :81-82);
 *   else:      L = min(C, T - p), last = (p + L == T) (:83, :44-46).
 * Kept from the reference on purpose: a valid reply without the ACK flag does
 * not advance p, and if it answered the last frame L still drops to 0; the
 * host's timeout (SEND_DATA) is what recomputes L and last from p.  Replies
 * after `end` are not judged, and with done set on entry none is: d_valid and
 * d_pointer are then all 0, end = n and the state is copied.
 * RUDP_ACK_CUMULATIVE (defined by this library, as the checksum is; the
 * reference never has two frames in flight) changes valid_i alone:
 *   valid_i = usable_i && expected <= ack_i <= isn + sent_chars &&
 *             ((ack_i - isn) % C == 0 || ack_i - isn == T)
 * where sent_chars (>= p + L, <= T) is what the host has sent so far; a sender
 * with several frames in flight that lost a reply takes the next one.
 *
 * rudp_ack_progress: the rule over decoded tables.  d_ack, d_flags as the
 * decode wrote them, d_usable_or_null[i] != 0 for a usable reply (NULL: all
 * usable); d_seq is checked like them and not read (the rule does not depend
 * on it; the closing datagram's ack_num is d_seq[end] + 1).  Outputs:
 *   d_valid[i]    u8: valid_i
 *   d_pointer[i]  u64: p after reply i
 * and both are 0 for i > end.  d_state_out (u64[4], may be d_state_in): the
 * state after reply `end`, or after all n.  d_info (u64[8]):
 *   [0] end (n when no valid reply has FIN)
 *   [1] the number of valid replies
 *   [2] characters newly acknowledged (p after - p before)
 *   [3] p after
 *   [4] first_anomaly: the index where the one-scan form stopped being exact
 *       and the sequential form took over (n when it never did; see DESIGN)
 *   [5] the next frame index ceil(p / C): the row of rudp_segment_utf8's table
 *       to send next (for p == T > 0 the header-only FIN row a caller appends)
 *   [6] done
 *   [7] 0, reserved
 * n == 0 copies the state, writes d_info and nothing else.  RUDP_EINVAL before
 * any HIP call: d_state_in, d_state_out or d_info NULL; isn above 65535;
 * chunk_chars outside [1, 16383]; a mode other than the two; sent_chars >
 * total_chars; with n > 0, d_seq, d_ack, d_flags, d_valid or d_pointer NULL.
 *
 * rudp_acknowledge: reply datagrams in, everything above and the closing
 * datagram out, in one call.  d_frames, frames_bytes, d_frame_off[n + 1],
 * len_hint, n, d_csum_in_or_null and layout as rudp_decode_varlen_checked
 * takes them; then the arguments of rudp_ack_progress.  Outputs through *out:
 *   seq, ack, flags, ok, csum_out_or_null
 *                 as rudp_decode_varlen_checked writes them
 *   usable        u8: 1 when ok is RUDP_OK_GOOD or RUDP_OK_UNVERIFIED.  A short
 *                 frame, a wrong checksum and bad offsets are not usable; UTF-8
 *                 validity is not required (wait_ack never reads the payload)
 *   valid, pointer, state_out[4] (may be d_state_in), info[8]
 *                 as rudp_ack_progress, with `usable` as its mask
 *   final_frame   `layout` bytes: Packet().to_byte() of the closing datagram
 *                 (for layout 7 with its RFC 1071 checksum in-band), written
 *                 only when end < n
 *   final_csum_or_null  u16[1]: its checksum, written with it
 *   status        u32, required: 0, or RUDP_ST_OFFSETS when a frame was
 *                 rejected for its offsets (it is not usable and none of its
 *                 bytes is read)
 * Every table is bit for bit what rudp_decode_varlen_checked, the usable rule
 * and rudp_ack_progress write when called one after another.  A batch of at
 * most 1024 replies in at most 32768 bytes and 261 bytes per reply is one
 * launch of one workgroup that reads the frames once; larger batches run the
 * decode, a usable pass, the rule's launches and a closing builder.  n == 0
 * copies the state, writes info and status = 0, and touches nothing else.
 * RUDP_EINVAL before any HIP call: out NULL; a layout other than 5 or 7; a
 * sideband d_csum_in with layout 7; the scalar checks of rudp_ack_progress;
 * d_state_in, state_out, info or status NULL; with n > 0, d_frame_off,
 * final_frame or any table other than csum_out_or_null NULL, or d_frames NULL
 * with frames_bytes > 0.
 */
#define RUDP_HAS_ACKNOWLEDGE 1
#define RUDP_ACK_EXACT 0
#define RUDP_ACK_CUMULATIVE 1
typedef struct rudp_acknowledged {
  uint16_t* seq;
  uint16_t* ack;
  uint8_t* flags;
  uint8_t* ok;
  uint16_t* csum_out_or_null;
  uint8_t* usable;
  uint8_t* valid;
  uint64_t* pointer;
  uint64_t* state_out;
  uint64_t* info;
  uint8_t* final_frame;
  uint16_t* final_csum_or_null;
  uint32_t* status;
} rudp_acknowledged;
RUDP_API int rudp_ack_progress(const uint16_t* d_seq, const uint16_t* d_ack, const uint8_t* d_flags,
                               const uint8_t* d_usable_or_null, uint64_t n, uint32_t isn, uint64_t total_chars,
                               uint32_t chunk_chars, int mode, uint64_t sent_chars, const uint64_t* d_state_in,
                               uint8_t* d_valid, uint64_t* d_pointer, uint64_t* d_state_out, uint64_t* d_info,
                               int device, void* hip_stream);
RUDP_API int rudp_acknowledge(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                              uint32_t len_hint, uint64_t n, const uint16_t* d_csum_in_or_null, uint32_t isn,
                              uint64_t total_chars, uint32_t chunk_chars, int mode, uint64_t sent_chars,
                              const uint64_t* d_state_in, const rudp_acknowledged* out, int layout, int device,
                              void* hip_stream);

/*
 * One reply batch judged for many transfers (added within ABI 8,
 * RUDP_HAS_ACK_FLOWS): rudp_ack_progress' rule for the reply datagrams of many
 * concurrent sends, the mirror image of rudp_accept_flows.  One call judges a
 * batch of at most RUDP_FLOWS_MAX_BATCH replies in one launch, with every
 * per-transfer constant and state in a device table.  Sync-free: asynchronous
 * on hip_stream, the host never waits, no temporaries, usable under stream
 * capture, no work proportional to the table.
 *
 * d_seq, d_ack, d_flags, d_usable_or_null and n as rudp_ack_progress takes
 * them; d_flow[i] (u32) is the slot of reply i's peer; mode is RUDP_ACK_EXACT
 * or RUDP_ACK_CUMULATIVE, for the whole call.  d_states is u64[n_flows][8],
 * read and written in place; a row is {p, L, last, done, isn, T, C, sent}:
 * words 0 to 3 are rudp_ack_progress' state, words 4 to 7 its scalars isn,
 * total_chars, chunk_chars and sent_chars.  The call writes only words 0 to 3,
 * and only of rows whose slot occurs in the batch; the host owns words 4 to 7
 * (in CUMULATIVE mode it updates sent of the flows it has sent to before the
 * call; sent is not read in EXACT mode).  A fresh transfer's row is
 * {0, min(C, T), L == T, 0, isn, T, C, 0}.
 *
 * Per slot the rule is exactly rudp_ack_progress' (its text above is the
 * definition, the quirks kept from the reference included), applied to the
 * slot's replies in arrival order with the row as d_state_in and as the
 * scalars, the slots independently.  Ignored: a reply with d_flow[i] ==
 * RUDP_FLOW_NONE; one with d_flow[i] >= n_flows, which sets RUDP_ST_FLOW; one
 * whose row has C == 0, an idle slot (an all-zero table is a table of idle
 * slots), silently; one whose row has isn > 65535, C > 16383 or, in
 * CUMULATIVE mode, sent > T, which sets RUDP_ST_FLOW_ROW.  An ignored reply
 * gets every per-reply output 0 and touches no row; the flow of an ignored row
 * is not among the active flows, and its replies go with the flowless ones in
 * d_order.  A flow whose row has done set on entry is listed but not judged:
 * valid = 0, end = n, the row unchanged.  A flow's first valid FIN ends it at
 * arrival index end_f: done becomes 1 and its later replies in this call are
 * not judged.
 *
 * Per-reply outputs, n entries each, in arrival order:
 *   d_valid[i]    u8: valid_i
 *   d_pointer[i]  u64: p of that reply's flow after the reply; 0 where the
 *                 reply was not judged
 * Grouping outputs, A = the distinct slots of the batch that were judged or
 * found done:
 *   d_order[n], d_order_off[0..A]
 *                 as rudp_accept_flows defines them: flow-major, ascending
 *                 slot, arrival order within a slot, the rest last (provide
 *                 n + 1 entries of d_order_off)
 *   d_flow_info   u64[A][8], ascending by slot (provide n rows): [0] slot
 *                 [1] end (arrival index; n: none) [2] valid replies
 *                 [3] characters newly acknowledged [4] p after [5] the next
 *                 frame index ceil(p / C) [6] done after [7] for a flow with
 *                 end < n closing_seq | closing_ack << 16, else 0:
 *                 closing_seq = (isn + p) mod 2^16 and closing_ack =
 *                 (seq_end + 1) mod 2^16, rudp_acknowledge's closing datagram
 *   d_info        u64[8]: [0] A [1] valid replies in all [2] E, the flows that
 *                 ended in this call [3] characters newly acknowledged in all
 *                 [4] replies outside the A runs [5] flows the kernel judged
 *                 sequentially (a diagnostic, not part of the contract)
 *                 [6..7] 0
 *   *d_status     required: 0, or RUDP_ST_FLOW | RUDP_ST_FLOW_ROW
 * Closing datagrams, with final_layout 5 or 7: d_final_frames receives E
 * datagrams of final_layout bytes at that stride, for the flows with end < n
 * in ascending slot order, each with flags 0x40, the fields above and, for
 * layout 7, its RFC 1071 checksum in-band; d_final_csum_or_null u16[E], the
 * checksums; d_final_flow u32[E], the index a into d_flow_info.  Provide n *
 * final_layout bytes and n entries; nothing is written at or past E *
 * final_layout.  With final_layout 0 these pointers may be NULL and nothing is
 * built.
 * Nothing is written past index A of d_order_off or past row A - 1 of
 * d_flow_info.  n == 0 writes d_info = 0 and *d_status = 0 and touches nothing
 * else.  n > RUDP_FLOWS_MAX_BATCH returns RUDP_ENOTSUP.  RUDP_EINVAL before any
 * HIP call: d_states, d_info or d_status NULL; n_flows 0 or above 2^32 - 2; a
 * mode other than the two; a final_layout other than 0, 5 or 7; with n > 0,
 * any other pointer NULL except d_usable_or_null, d_final_csum_or_null and,
 * with final_layout 0, the final tables.
 */
#define RUDP_HAS_ACK_FLOWS 1
#define RUDP_ST_FLOW_ROW 512u /* ack_flows: a row with isn > 65535, C > 16383 or (CUMULATIVE) sent > T */
RUDP_API int rudp_ack_flows(const uint16_t* d_seq, const uint16_t* d_ack, const uint8_t* d_flags,
                            const uint8_t* d_usable_or_null, const uint32_t* d_flow, uint64_t n, int mode,
                            uint64_t* d_states, uint64_t n_flows,
                            uint8_t* d_valid, uint64_t* d_pointer, uint32_t* d_order, uint32_t* d_order_off,
                            uint64_t* d_flow_info, uint64_t* d_info, uint32_t* d_status,
                            int final_layout, uint8_t* d_final_frames, uint16_t* d_final_csum_or_null,
                            uint32_t* d_final_flow, int device, void* hip_stream);

/*
 * Bounds of a variable-length batch, computed on the device (argument checks
 * the varlen entry points need before they can size or trust a buffer; the
 * reference has no batch and so no counterpart).  Synchronous on hip_stream.
 * rudp_varlen_bounds: h_out[0..4] = min len, max len, sum of len, min
 * payload_off, max(payload_off + len); without offsets [3] = 0, [4] = sum.
 * len[] is read as u32 (a negative int32 length shows as > 65535).
 * rudp_frame_off_bounds: over d_frame_off[0..n], h_out[0..2] = min, max and
 * the number of i < n with d_frame_off[i+1] < d_frame_off[i] (0 = valid
 * offsets for rudp_decode; min and max are then the first and last).
 */
RUDP_API int rudp_varlen_bounds(const uint32_t* d_len, const int64_t* d_payload_off_or_null, uint64_t n,
                       int64_t* h_out, int device, void* hip_stream);
RUDP_API int rudp_frame_off_bounds(const int64_t* d_frame_off, uint64_t n, int64_t* h_out, int device,
                          void* hip_stream);

/*
 * Strict UTF-8 check of each frame's payload: d_valid[i] = 1 when
 * Packet(frame).get_payload() would return (utils/packet.py:68-73: empty
 * payload -> None; else bytes.decode(), strict UTF-8), 0 when it would raise
 * UnicodeDecodeError.  Frames as in rudp_decode (fixed stride or offsets;
 * with offsets frame_len is a typical-length hint, as there).
 */
RUDP_API int rudp_validate_utf8(const uint8_t* d_frames, const uint64_t* d_frame_off_or_null,
                       uint32_t frame_len, uint64_t n, int layout, uint8_t* d_valid, int device,
                       void* hip_stream);

/*
 * Retransmission detection of the reference proxy (proxy.py:90: `packet in
 * self.packets`, a list of the last Proxy.MAX_MEMORY = 500 packets,
 * proxy.py:17, :92-94) over a batch of frames in arrival order:
 * d_dup[i] = 1 iff frame i equals (Packet.__eq__, utils/packet.py:83-86: same
 * get_hex(), so an empty datagram equals 00 00 00 00 00) one of frames
 * max(0, i - window) .. i-1.  window <= 4096 (the proxy uses 500).  To carry
 * history across batches, prepend the previous batch's last `window` frames.
 * Frames as in rudp_decode (fixed stride or n+1 offsets; with offsets
 * frame_len is a typical-length hint that picks lanes per frame).
 */
RUDP_API int rudp_dedup_window(const uint8_t* d_frames, const uint64_t* d_frame_off_or_null,
                      uint32_t frame_len, uint64_t n, uint32_t window, uint8_t* d_dup, int device,
                      void* hip_stream);

/*
 * rudp_dedup_window over packed frames with the argument check on the device
 * (ABI 5; the sync-free form the Python layer uses): every frame checks its
 * own pair of offsets against [0, frames_bytes]; a frame whose offsets are
 * decreasing or past the buffer gets d_dup = RUDP_DUP_BAD_OFFSETS, none of its
 * bytes is read, and it equals no other frame.  len_hint: the mean frame
 * length (picks lanes per frame, never the result).
 */
#define RUDP_DUP_BAD_OFFSETS 2
RUDP_API int rudp_dedup_window_checked(const uint8_t* d_frames, uint64_t frames_bytes, const uint64_t* d_frame_off,
                              uint32_t len_hint, uint64_t n, uint32_t window, uint8_t* d_dup, int device,
                              void* hip_stream);

/*
 * The proxy's retransmission count over a datagram stream (ABI 6; proxy.py:79-94:
 * every datagram is checked against the last Proxy.MAX_MEMORY = 500 of both
 * directions, proxy.py:17, :90-94, and counted per side).  The history stays
 * on the device between batches and nothing here waits for the GPU:
 * rudp_dedup_stream_push copies a batch of host frames (packed, n + 1
 * offsets; any host memory, the caller may reuse it once the call returns)
 * behind the history, flags it with rudp_dedup_window_checked's rule, adds
 * the flags to per-side counters (h_side_or_null[i] = 0 or 1; NULL: all 0),
 * optionally copies the batch's flags to d_dup_or_null (n bytes, device), and
 * keeps the last `window` datagrams, all on the stream given at creation.
 * rudp_dedup_stream_counts synchronizes and returns the two counters.
 * window <= 4096; a batch holds at most max_batch datagrams of at most
 * max_frame bytes each.  Thread-safe: push and counts may come from different
 * threads (a relay thread pushing, another reading its counters); the object
 * serializes them.  destroy must be the object's last call.
 */
typedef struct rudp_dedup_stream rudp_dedup_stream;
RUDP_API int rudp_dedup_stream_create(uint32_t window, uint32_t max_batch, uint32_t max_frame, int device,
                                      void* hip_stream, rudp_dedup_stream** out);
RUDP_API int rudp_dedup_stream_push(rudp_dedup_stream* st, const uint8_t* h_frames, const uint64_t* h_frame_off,
                                    uint64_t n, const uint8_t* h_side_or_null, uint8_t* d_dup_or_null);
RUDP_API int rudp_dedup_stream_counts(rudp_dedup_stream* st, uint64_t* h_counts);
RUDP_API int rudp_dedup_stream_destroy(rudp_dedup_stream* st);

/*
 * Batched UDP socket I/O (host only, no device work): the reference moves one
 * datagram per system call (sendto, utils/reliableUDP.py:61; recvfrom(1024),
 * :67, :118; proxy.py:129).  These move up to 1024 per call (sendmmsg /
 * recvmmsg) between a socket and caller-owned host buffers, in the packed
 * frames + offsets layout of rudp_encode_varlen / variable-length rudp_decode.
 *
 * rudp_udp_recv_batch: waits up to timeout_ms (-1 forever, 0 not at all) for
 * a first datagram, then drains up to min(max_msgs, cap_bytes / slot_bytes)
 * without blocking.  A datagram longer than slot_bytes is truncated (as the
 * reference's recvfrom(1024) truncates).  Frames are packed from h_frames[0];
 * h_frame_off receives count+1 offsets.  Returns the count (0 on timeout) or
 * a negative errno.
 * rudp_udp_send_batch: sends frames [h_frame_off[i], h_frame_off[i+1]) for
 * i < n to ip:port.  Returns the count sent or a negative errno.
 */
RUDP_API int rudp_udp_recv_batch(int fd, uint8_t* h_frames, uint64_t cap_bytes, uint32_t slot_bytes,
                        uint32_t max_msgs, uint64_t* h_frame_off, int timeout_ms);
RUDP_API int rudp_udp_send_batch(int fd, const uint8_t* h_frames, const uint64_t* h_frame_off, uint64_t n,
                        const char* ip, uint16_t port);

/*
 * The same for a relay in the reference proxy's role, which forwards every
 * datagram by its source address (proxy.py:129-145) over one socket.  An
 * IPv4 endpoint travels as one integer: address (host byte order) << 16 | port.
 * rudp_udp_recv_batch_from: as rudp_udp_recv_batch, and h_src_or_null[i]
 *   receives datagram i's source (0 for a non-IPv4 source).
 * rudp_udp_send_batch_to: sends frame i to h_dst[i] (per_datagram != 0) or
 *   every frame to h_dst[0].  Returns the count sent or a negative errno.
 */
RUDP_API int rudp_udp_recv_batch_from(int fd, uint8_t* h_frames, uint64_t cap_bytes, uint32_t slot_bytes,
                             uint32_t max_msgs, uint64_t* h_frame_off, uint64_t* h_src_or_null,
                             int timeout_ms);
RUDP_API int rudp_udp_send_batch_to(int fd, const uint8_t* h_frames, const uint64_t* h_frame_off, uint64_t n,
                           const uint64_t* h_dst, int per_datagram);

/*
 * Host-memory conveniences: same semantics, host pointers in and out.
 * Staged through a ring of device slots in chunks, with H2D, kernel and D2H
 * on three streams chained by events so the three overlap.  Synchronous.  These model the reference's
 * real boundary, a UDP socket buffer in host memory (utils/reliableUDP.py:61,
 * :67, :118).  Pinned (page-locked) host buffers copy at the link's rate;
 * pageable ones through the runtime's bounce buffers, at about half of it.
 *
 * rudp_decode_host (ABI 7: h_valid_or_null added): rudp_decode_utf8 of
 *   fixed-length frames in host memory -- the reference's receive, Packet(data)
 *   + get_header_field + get_payload() per datagram (utils/reliableUDP.py:118-121,
 *   utils/packet.py:16, :29-40, :68-73) -- with h_valid_or_null[i] its strict
 *   UTF-8 answer, judged in the decode pass (NULL: not computed).
 * rudp_decode_varlen_host (ABI 7): rudp_decode_varlen_utf8 of packed frames
 *   in host memory (a recvmmsg batch: frame i = h_frames[h_frame_off[i],
 *   h_frame_off[i + 1]), frames_bytes = size of h_frames), with every frame's
 *   offsets checked against frames_bytes as there (a rejected frame gets
 *   h_ok = RUDP_OK_BAD_OFFSETS and h_valid = 0, and *h_status_or_null =
 *   RUDP_ST_OFFSETS); the payload is zero-copy (frame i's bytes from
 *   layout on).  len_hint: the typical frame length (0: frames_bytes / n).
 *   Each chunk stages the byte range its offsets span: one valid frame over
 *   host_stage bytes (128 MiB) is refused with RUDP_ENOTSUP.
 * rudp_encode_varlen_host (ABI 7): rudp_encode_varlen of packed payloads in
 *   host memory (h_in->payload_off must be NULL; h_in->payload_len is a hint
 *   of the typical length) to packed frames in host memory -- the send side,
 *   Packet() + set_header_field + set_payload + to_byte() per datagram
 *   (utils/reliableUDP.py:53-61, utils/packet.py:43-65, :76-81).
 *   h_frame_off receives n + 1 offsets (the exclusive scan of len[i] +
 *   layout).  Every length (<= 65535), sum(len) == payload_bytes (the size
 *   of h_in->payload) and frames_cap (>= sum(len) + n * layout) are checked
 *   before any frame byte is written: a bad batch returns RUDP_EINVAL and
 *   h_frames and h_csum_or_null are untouched.  The host checks the lengths
 *   before it enqueues any work, except for a batch of small frames (mean
 *   payload under 16 B) whose every array is pinned: that one runs as one
 *   checked device encode over PCIe, whose first pass makes the same checks
 *   (h_frame_off is then left unspecified on a bad batch).
 */
RUDP_API int rudp_encode_host(const rudp_batch* h_in, uint8_t* h_frames, uint16_t* h_csum_or_null,
                     int layout, int device);
RUDP_API int rudp_decode_host(const uint8_t* h_frames, uint32_t frame_len, uint64_t n,
                     const uint16_t* h_csum_in_or_null, uint16_t* h_seq, uint16_t* h_ack,
                     uint8_t* h_flags, uint8_t* h_ok, uint16_t* h_csum_out_or_null,
                     uint8_t* h_payload_out_or_null, uint8_t* h_valid_or_null, int layout, int device);
RUDP_API int rudp_decode_varlen_host(const uint8_t* h_frames, uint64_t frames_bytes, const uint64_t* h_frame_off,
                                     uint32_t len_hint, uint64_t n, const uint16_t* h_csum_in_or_null,
                                     uint16_t* h_seq, uint16_t* h_ack, uint8_t* h_flags, uint8_t* h_ok,
                                     uint16_t* h_csum_out_or_null, uint8_t* h_valid_or_null,
                                     uint32_t* h_status_or_null, int layout, int device);
RUDP_API int rudp_encode_varlen_host(const rudp_batch* h_in, uint64_t payload_bytes, uint8_t* h_frames,
                                     uint64_t frames_cap, uint64_t* h_frame_off, uint16_t* h_csum_or_null,
                                     int layout, int device);

/*
 * Deterministic synthetic batch, generated on the device:
 * packet i (global index first_index + local index) gets
 *   seq = (isn + i) mod 2^16, isn in [1, 5000]   (utils/reliableUDP.py:41, :54)
 *   ack = splitmix u16, flags uniform over {00,80,20,A0,40,60}
 *   payload bytes from splitmix64, masked to 0x00-0x7F when ascii != 0.
 * The same definition is restated on the CPU in oracle/synth.py.
 */
RUDP_API int rudp_synth(uint64_t seed, uint64_t first_index, uint64_t n, uint32_t payload_len,
               int ascii, uint16_t* d_seq, uint16_t* d_ack, uint8_t* d_flags,
               uint8_t* d_payload, int device, void* hip_stream);

RUDP_API int rudp_device_count(int* count);
RUDP_API const char* rudp_last_error(void);
RUDP_API int rudp_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* RUDP_H_ */
