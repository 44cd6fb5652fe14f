// The host rules of the ticketed queries (query_async.hip: edynhip_raycast_submit, edynhip_query_aabb_submit, edynhip_query_poll,
// edynhip_*_collect, edynhip_query_release), each written once: the table of outstanding tickets, and what a submit's arguments must
// look like. Plain C++ over arrays - no HIP, no context - so every rule is tested on a machine without a GPU
// (tests/cpp/query_tickets.cpp).
#pragma once
#include "../../include/edynhip.h"
#include <cstddef>
#include <cstdint>

namespace eh {

enum { TICKET_FREE = 0, TICKET_RAYS = 1, TICKET_BOXES = 2 };
constexpr uint32_t kWantAll = EDYNHIP_WANT_PROCEDURAL | EDYNHIP_WANT_NON_PROCEDURAL | EDYNHIP_WANT_ISLANDS | EDYNHIP_WANT_OF_INTEREST;

// At most EDYNHIP_QUERY_TICKETS_MAX tickets are outstanding, one per slot; a slot keeps its buffers when its ticket goes, the next
// ticket that takes the slot finds them there. Ticket values count up from 1 and are never reused (0 is no ticket), so a released
// ticket, or a number that was never handed out, is found in no slot.
struct TicketTable {
    struct Slot { uint64_t ticket = 0; int kind = TICKET_FREE; };
    Slot slot[EDYNHIP_QUERY_TICKETS_MAX];
    uint64_t next = 1;

    // the lowest free slot takes a new ticket; -1: all slots are taken (nothing changes, no ticket value is spent)
    int acquire(int kind, uint64_t *ticket) {
        for (int s = 0; s < (int)EDYNHIP_QUERY_TICKETS_MAX; ++s)
            if (slot[s].kind == TICKET_FREE) {
                slot[s].ticket = next++;
                slot[s].kind = kind;
                *ticket = slot[s].ticket;
                return s;
            }
        return -1;
    }
    // the slot of an outstanding ticket, or -1
    int find(uint64_t ticket) const {
        if (ticket == 0) return -1;
        for (int s = 0; s < (int)EDYNHIP_QUERY_TICKETS_MAX; ++s)
            if (slot[s].kind != TICKET_FREE && slot[s].ticket == ticket) return s;
        return -1;
    }
    // false: the ticket is not outstanding
    bool release(uint64_t ticket) {
        const int s = find(ticket);
        if (s < 0) return false;
        slot[s] = Slot();
        return true;
    }
    uint32_t outstanding() const {
        uint32_t k = 0;
        for (const Slot &s : slot) k += s.kind != TICKET_FREE;
        return k;
    }
};

// The sequence number a ticket publishes when its results are in place (query_async.hip k_qt_publish): the low word of the ticket,
// with 0 - what a fresh slot holds - left out. A slot's consecutive tickets differ, so do their numbers (2^32 - 1 submits apart aside).
inline uint32_t ticket_sequence(uint64_t ticket) {
    const uint32_t v = (uint32_t)ticket;
    return v ? v : 0x80000000u;
}

// ignore_offsets[n + 1] of edynhip_raycast_submit: the list of ray i is ignore_ids[offsets[i] .. offsets[i + 1]). They must not
// descend (a list of negative length), and a non-empty total needs the ids. NULL offsets: no ray ignores anything.
inline bool ignore_offsets_ok(uint32_t n, const uint32_t *offsets, const uint32_t *ids) {
    if (!offsets) return true;
    for (uint32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return false;
    return offsets[n] == offsets[0] || ids != nullptr;
}
// want[n] of edynhip_query_aabb_submit: EDYNHIP_WANT_* bits only
inline bool want_masks_ok(uint32_t n, const uint8_t *want) {
    if (n && !want) return false;
    for (uint32_t i = 0; i < n; ++i)
        if (want[i] & ~kWantAll) return false;
    return true;
}
inline uint32_t want_union(uint32_t n, const uint8_t *want) {
    uint32_t u = 0;
    for (uint32_t i = 0; i < n; ++i) u |= want[i];
    return u;
}
// the flag bits a submit accepts are those of its synchronous twin
inline bool ray_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)EDYNHIP_RAYCAST_BRUTE_FORCE) == 0; }
inline bool box_flags_ok(uint32_t flags) { return (flags & ~(uint32_t)EDYNHIP_QUERY_BRUTE_FORCE) == 0; }

// collect of a box ticket: the lists fit when the 64-bit total is within the capacity the ticket was submitted with
inline bool lists_fit(uint64_t total, uint32_t ids_capacity) { return total <= (uint64_t)ids_capacity; }

}  // namespace eh
