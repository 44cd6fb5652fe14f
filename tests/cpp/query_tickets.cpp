// The host rules of the ticketed queries (edyn_amd/csrc/query_tickets.hpp): the table of outstanding tickets and the argument checks
// of edynhip_raycast_submit / edynhip_query_aabb_submit, against values written from the rules' statements. Plain C++: no HIP, no
// library, a main of its own.
#include "../../edyn_amd/csrc/query_tickets.hpp"
#include <cstdio>
#include <set>
#include <vector>

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

using namespace eh;
constexpr int kMax = EDYNHIP_QUERY_TICKETS_MAX;

static void limits() {
    TicketTable t;
    CHECK(t.outstanding() == 0);
    uint64_t id[kMax] = {0};
    std::set<int> slots;
    for (int k = 0; k < kMax; ++k) {
        const int s = t.acquire(k & 1 ? TICKET_BOXES : TICKET_RAYS, &id[k]);
        CHECK(s >= 0 && s < kMax);
        slots.insert(s);
        CHECK(id[k] == (uint64_t)k + 1);   // values count up from 1
    }
    CHECK((int)slots.size() == kMax && t.outstanding() == (uint32_t)kMax);
    // the ninth: refused, no value spent, nobody disturbed
    uint64_t ninth = 77;
    const uint64_t next = t.next;
    CHECK(t.acquire(TICKET_RAYS, &ninth) == -1);
    CHECK(ninth == 77 && t.next == next && t.outstanding() == (uint32_t)kMax);
    for (int k = 0; k < kMax; ++k) {
        const int s = t.find(id[k]);
        CHECK(s >= 0 && t.slot[s].ticket == id[k] && t.slot[s].kind == (k & 1 ? TICKET_BOXES : TICKET_RAYS));
    }
}

static void stale_and_unknown() {
    TicketTable t;
    uint64_t a = 0, b = 0;
    CHECK(t.find(0) == -1 && t.find(1) == -1 && t.find(~0ull) == -1);   // nothing was handed out yet; 0 is no ticket
    CHECK(!t.release(0) && !t.release(1));
    const int sa = t.acquire(TICKET_RAYS, &a);
    CHECK(t.find(a) == sa && t.find(a + 1) == -1);
    CHECK(t.release(a));
    CHECK(t.find(a) == -1 && !t.release(a));   // stale: found nowhere, released once only
    const int sb = t.acquire(TICKET_BOXES, &b);
    CHECK(sb == sa);                            // the slot (and its buffers) is taken again ...
    CHECK(b != a && b == a + 1);                // ... under a new value
    CHECK(t.find(a) == -1 && t.find(b) == sb);
    CHECK(t.find(0) == -1);                     // a free slot's ticket field (0) is never a match
}

static void any_order_and_refill() {
    TicketTable t;
    uint64_t id[kMax];
    int slot[kMax];
    for (int k = 0; k < kMax; ++k) slot[k] = t.acquire(TICKET_RAYS, &id[k]);
    // collected (found) and released in an order of their own
    const int order[kMax] = {5, 0, 7, 2, 6, 1, 3, 4};
    for (int i = 0; i < kMax; ++i) {
        const int k = order[i];
        CHECK(t.find(id[k]) == slot[k]);
        CHECK(t.release(id[k]));
        CHECK(t.outstanding() == (uint32_t)(kMax - 1 - i));
        for (int j = i + 1; j < kMax; ++j) CHECK(t.find(id[order[j]]) == slot[order[j]]);   // the others stay
    }
    // refill: the lowest free slot first, values go on counting
    std::set<uint64_t> seen(id, id + kMax);
    for (int k = 0; k < kMax; ++k) {
        uint64_t v = 0;
        CHECK(t.acquire(TICKET_BOXES, &v) == k);
        CHECK(seen.insert(v).second && v == (uint64_t)kMax + 1 + k);
    }
    uint64_t v = 0;
    CHECK(t.acquire(TICKET_BOXES, &v) == -1);
    // a hole in the middle is the one that fills
    CHECK(t.release((uint64_t)kMax + 1 + 3));
    CHECK(t.acquire(TICKET_RAYS, &v) == 3 && v == 2 * (uint64_t)kMax + 1);
    // long run: values never repeat
    for (int r = 0; r < 1000; ++r) {
        CHECK(t.release(v));
        CHECK(t.acquire(TICKET_RAYS, &v) == 3);
        CHECK(seen.insert(v).second);
    }
}

static void sequences() {
    CHECK(ticket_sequence(1) == 1 && ticket_sequence(0xFFFFFFFFull) == 0xFFFFFFFFu);
    CHECK(ticket_sequence(0x100000000ull) != 0);   // a fresh slot holds 0: no ticket publishes it
    CHECK(ticket_sequence(0x100000001ull) == 1);
    for (uint64_t v = 1; v < 64; ++v) CHECK(ticket_sequence(v) != ticket_sequence(v + 1));
}

static void offsets_and_masks() {
    const uint32_t ids[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    { const uint32_t off[4] = {0, 2, 2, 8}; CHECK(ignore_offsets_ok(3, off, ids)); }       // an empty list in the middle
    { const uint32_t off[4] = {3, 3, 5, 8}; CHECK(ignore_offsets_ok(3, off, ids)); }       // need not start at 0
    { const uint32_t off[4] = {0, 2, 1, 8}; CHECK(!ignore_offsets_ok(3, off, ids)); }      // descends
    { const uint32_t off[4] = {4, 2, 2, 2}; CHECK(!ignore_offsets_ok(3, off, ids)); }      // descends at once
    { const uint32_t off[4] = {0, 0, 0, 0}; CHECK(ignore_offsets_ok(3, off, nullptr)); }   // no ids named: none needed
    { const uint32_t off[4] = {0, 0, 0, 1}; CHECK(!ignore_offsets_ok(3, off, nullptr)); }  // ids named but missing
    { const uint32_t off[1] = {5}; CHECK(ignore_offsets_ok(0, off, nullptr)); }            // no rays
    CHECK(ignore_offsets_ok(3, nullptr, nullptr) && ignore_offsets_ok(0, nullptr, nullptr));
    { const uint32_t off[3] = {0, 0xFFFFFFFFu, 0xFFFFFFFFu}; CHECK(ignore_offsets_ok(2, off, ids)); }

    std::vector<uint8_t> w;
    for (int m = 0; m < 16; ++m) w.push_back((uint8_t)m);
    CHECK(want_masks_ok(16, w.data()) && want_union(16, w.data()) == 15u);
    CHECK(want_masks_ok(0, nullptr) && !want_masks_ok(1, nullptr));
    for (int bit = 4; bit < 8; ++bit) {
        std::vector<uint8_t> bad = w;
        bad[9] |= (uint8_t)(1u << bit);
        CHECK(!want_masks_ok(16, bad.data()));
    }
    { const uint8_t one[3] = {EDYNHIP_WANT_ISLANDS, 0, EDYNHIP_WANT_OF_INTEREST}; CHECK(want_union(3, one) == 12u && want_masks_ok(3, one)); }
    CHECK(kWantAll == 15u);

    CHECK(ray_flags_ok(0) && ray_flags_ok(EDYNHIP_RAYCAST_BRUTE_FORCE) && !ray_flags_ok(2) && !ray_flags_ok(0x80000000u));
    CHECK(box_flags_ok(0) && box_flags_ok(EDYNHIP_QUERY_BRUTE_FORCE) && !box_flags_ok(2) && !box_flags_ok(3));
    CHECK(lists_fit(0, 0) && lists_fit(7, 7) && !lists_fit(8, 7) && !lists_fit(0x100000000ull, 0xFFFFFFFFu) && lists_fit(0xFFFFFFFFull, 0xFFFFFFFFu));
}

int main() {
    limits();
    stale_and_unknown();
    any_order_and_refill();
    sequences();
    offsets_and_masks();
    if (failures) { std::printf("QUERY_TICKETS_FAILED %d\n", failures); return 1; }
    std::printf("QUERY_TICKETS_OK\n");
    return 0;
}
