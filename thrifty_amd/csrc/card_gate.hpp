// The carrier gate (fastcard's job: raw capture -> carrier verdict -> .card): declarations of
// card_gate.hip.  The carrier stage itself is the detectors' (launch_carrier_*, detect_common.hpp);
// what is added here is cardet's power-domain verdict with an order-preserving list of the blocks
// that pass, and the base64 ENCODE of those blocks -- the mirror image of card_ingest.hip.
#pragma once
#include "host_internal.hpp"

// A gate handle (thr_create_ex, THR_VARIANT_GATE) is a thr_handle with the gate's state behind it.  The tag
// is dev.variant: create_body writes THR_VARIANT_GATE there for the handles it allocates as thr_gate_handle
// and for no other (the carrier kernels never read that field).
struct thr_gate_handle : thr_handle {
    float gate_c = 0, gate_s = 0;             // pass when max > c + s * noise (power domain, float32 like cardet's)
    Dev<int> d_gate_pos;                      // [max_batch] positions of the passed blocks, input order
    Dev<int> d_gate_count;                    // [2]: passed blocks of the chunk, invalid base64 payloads
    Pinned<int> h_gate_count;                 // pinned twin
    Dev<thr_record> d_gate_rec;               // [max_batch]
    Dev<unsigned char> d_gate_slots;          // [chunk][slot_stride] base64 of the passed blocks
    Pinned<char> h_gate_slots;                // pinned twin: the device-to-host copy is count * slot_stride bytes
    Dev<unsigned char> d_gate_text;           // .card input: the chunk's text
    Dev<long long> d_gate_off;                // [2 * max_batch]: block indices, payload offsets
};
inline bool thr_is_gate(const thr_handle* h) { return h->dev.variant == THR_VARIANT_GATE; }
inline thr_gate_handle* thr_gate_of(thr_handle* h) {
    return thr_is_gate(h) ? static_cast<thr_gate_handle*>(h) : nullptr;
}

namespace thr {

// A passed block's slot in the encode output: payload_chars base64 characters, '\n', then unwritten
// bytes up to the next multiple of 16 (every 16-character group of every slot is one aligned store).
inline size_t gate_payload_chars(int block_len) { return ((size_t(block_len) * 2 + 2) / 3) * 4; }
inline size_t gate_slot_stride(int block_len) { return (gate_payload_chars(block_len) + 1 + 15) & ~size_t(15); }

// cardet_detect (fastcard cardet.c:7-41) for n_blocks blocks from the carrier stage's statistics:
// records, the positions of the passed blocks in input order, and their count.  One workgroup.
hipError_t launch_gate_verdict(const CarStats* d_stats, int n_blocks, int fft_len, float thr_const,
                               float thr_snr, const long long* d_block_idx, long long first_idx,
                               thr_record* d_rec, int* d_pos, int* d_count, hipStream_t stream);

// base64 of the 2 * block_len bytes of every listed block, read where they lie
// (samples + pos[s] * blk_stride, 4-byte aligned), into slot s of d_out.  The grid covers
// max_slots; slots at or above *d_count return at once.
hipError_t launch_b64_encode(const unsigned char* d_samples, unsigned long long blk_stride, int block_len,
                             const int* d_pos, const int* d_count, int max_slots, unsigned char* d_out,
                             hipStream_t stream);

}  // namespace thr
