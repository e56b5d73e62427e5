// The host part of csrc/plane_views.h (the pair test, the byte range of a plane, the checks of a plane and the overlap rule with their messages) under the host
// sanitizers.  A program of its own: built with -fsanitize=address,undefined on the host side and run directly -- never through Python, never on a GPU.  It
// includes that header alone, with a plane struct of its own, and makes no HIP call: every pointer here is only compared.
#include <stdlib.h>
#include <string.h>

#include "../head_detector_amd/csrc/plane_views.h"

using namespace planes;

struct Plane {  // the fields the header asks for, in an order of its own
    int32_t src_step, dst_step;
    const uint8_t* src_dev;
    uint8_t* dst_dev;
    int64_t src_pitch, dst_pitch;
};

static int failures = 0;
static char msg[400];

#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("line %d: %s (message: %s)\n", __LINE__, #cond, msg); \
            ++failures;                                                  \
        }                                                                \
    } while (0)

static Plane plane(uint8_t* src, uint8_t* dst, int64_t sp, int64_t dp, int ss, int ds) {
    Plane q = {};
    q.src_dev = src, q.dst_dev = dst, q.src_pitch = sp, q.dst_pitch = dp, q.src_step = ss, q.dst_step = ds;
    return q;
}

// the whole message of a refusal, or "" if the plane is taken
static const char* one(const Plane& q, int64_t pw, int max_step, const char* label) {
    msg[0] = 0;
    const char* m = check_plane(q, pw, max_step, "who", label, msg, sizeof(msg));
    EXPECT(m == nullptr || m == msg);
    return m ? m : "";
}

static const char* all(const Plane* p, int n, const int64_t* pw, const int64_t* ph, const char* const* labels) {
    msg[0] = 0;
    const char* m = check_overlap(p, n, pw, ph, "who", labels, msg, sizeof(msg));
    EXPECT(m == nullptr || m == msg);
    return m ? m : "";
}

int main() {
    uint8_t* mem = (uint8_t*)malloc(1 << 16);  // only its addresses are used
    uint8_t* even = mem + ((uintptr_t)mem & 1);
    // ---- pair_of: two step-2 planes are the bytes of one even-aligned 16-bit pair ----
    EXPECT(pair_of(even, even + 1, 64, 64, 2, 2) == 1);      // the first plane holds the lower bytes, at an even address
    EXPECT(pair_of(even + 1, even, 64, 64, 2, 2) == 2);      // ... the second one does
    EXPECT(pair_of(even + 1, even + 2, 64, 64, 2, 2) == 0);  // the lower byte at an odd address, either order: two planes
    EXPECT(pair_of(even + 2, even + 1, 64, 64, 2, 2) == 0);
    EXPECT(pair_of(even, even + 1, 64, 66, 2, 2) == 0 && pair_of(even + 1, even, 66, 64, 2, 2) == 0);  // unequal pitches
    EXPECT(pair_of(even, even + 1, 63, 63, 2, 2) == 0 && pair_of(even + 1, even, 65, 65, 2, 2) == 0);  // an odd pitch: every other row is misaligned
    EXPECT(pair_of(even, even + 1, 64, 64, 1, 2) == 0 && pair_of(even, even + 1, 64, 64, 2, 1) == 0 && pair_of(even, even + 1, 64, 64, 1, 1) == 0);  // a step of 1
    EXPECT(pair_of(even, even + 1, 64, 64, 3, 3) == 0 && pair_of(even, even + 3, 64, 64, 2, 2) == 0 && pair_of(even, even, 64, 64, 2, 2) == 0);
    EXPECT(pair_of(even, even + 1, (int64_t)1 << 40, (int64_t)1 << 40, 2, 2) == 1);

    // ---- plane_range: [a, b) ends behind the last sample of the last row ----
    uintptr_t a, b;
    plane_range(mem, 1, 1, 1, 1, a, b);
    EXPECT(a == (uintptr_t)mem && b == a + 1);
    plane_range(mem, 1 << 20, 3, 1, 1, a, b);  // one sample: neither the pitch nor the step counts
    EXPECT(b == a + 1);
    plane_range(mem + 7, 40, 2, 15, 10, a, b);  // pitched, step 2: 9 whole rows, then 14 steps and the sample
    EXPECT(a == (uintptr_t)mem + 7 && b == a + 9 * 40 + 14 * 2 + 1);
    plane_range(mem, (int64_t)1 << 40, 2, 32767, 32767, a, b);  // the largest plane the checks take: no overflow
    EXPECT(b - a == (uintptr_t)32766 * ((uintptr_t)1 << 40) + 32766 * 2 + 1);

    // ---- in_place, chan_of ----
    Plane q = plane(mem, mem, 32, 32, 2, 2);
    EXPECT(in_place(q));
    q.dst_pitch = 34;
    EXPECT(!in_place(q));
    q = plane(mem, mem, 32, 32, 2, 1);
    EXPECT(!in_place(q));
    q = plane(mem, mem + 1, 32, 32, 2, 2);
    EXPECT(!in_place(q));
    q = plane(mem + 3, mem + 5, 32, 48, 1, 2);
    const Chan c = chan_of(q);
    EXPECT(c.src == mem + 3 && c.dst == mem + 5 && c.spitch == 32 && c.dpitch == 48 && c.sstep == 1 && c.dstep == 2);

    // ---- one plane: every message, with both styles of label and both step ranges ----
    const Plane ok = plane(mem, mem + 4096, 32, 40, 2, 1);  // 15 samples a row
    EXPECT(!*one(ok, 15, 2, "U") && !*one(ok, 15, 3, "1"));
    q = ok, q.src_dev = nullptr;
    EXPECT(strstr(one(q, 15, 2, "Y"), "who: plane Y: null plane (src_dev ") == msg && strstr(one(q, 15, 3, "0"), "who: plane 0: null plane (src_dev ") == msg);
    q = ok, q.dst_dev = nullptr;
    EXPECT(strstr(one(q, 15, 2, "V"), "who: plane V: null plane (src_dev "));
    q = ok, q.src_step = 3;
    EXPECT(!strcmp(one(q, 15, 2, "U"), "who: plane U: steps 3 and 1 are not 1 or 2"));
    q.src_pitch = 43;
    EXPECT(!*one(q, 15, 3, "1"));  // 14 * 3 + 1 bytes
    q.src_step = 4;
    EXPECT(!strcmp(one(q, 15, 3, "1"), "who: plane 1: steps 4 and 1 are not 1, 2 or 3"));
    q = ok, q.dst_step = 0;
    EXPECT(!strcmp(one(q, 15, 2, "Y"), "who: plane Y: steps 2 and 0 are not 1 or 2") && !strcmp(one(q, 15, 3, "2"), "who: plane 2: steps 2 and 0 are not 1, 2 or 3"));
    q = ok, q.src_pitch = 28;
    EXPECT(!strcmp(one(q, 15, 2, "U"), "who: plane U: src_pitch 28 outside 29 .. 2^40") && !strcmp(one(q, 15, 3, "1"), "who: plane 1: src_pitch 28 outside 29 .. 2^40"));
    q.src_pitch = 29;
    EXPECT(!*one(q, 15, 2, "U"));
    q = ok, q.dst_pitch = 14;
    EXPECT(!strcmp(one(q, 15, 2, "V"), "who: plane V: dst_pitch 14 outside 15 .. 2^40") && !strcmp(one(q, 15, 3, "2"), "who: plane 2: dst_pitch 14 outside 15 .. 2^40"));
    q = ok, q.dst_pitch = ((int64_t)1 << 40) + 1;
    EXPECT(!strcmp(one(q, 15, 2, "Y"), "who: plane Y: dst_pitch 1099511627777 outside 15 .. 2^40"));
    q.dst_pitch = (int64_t)1 << 40;
    EXPECT(!*one(q, 15, 2, "Y"));
    q = ok, q.src_step = 0, q.src_pitch = 0, q.src_dev = nullptr;  // the first refusal is the one reported
    EXPECT(strstr(one(q, 15, 2, "Y"), "null plane"));
    q.src_dev = mem;
    EXPECT(strstr(one(q, 15, 2, "Y"), "steps 0 and 1"));
    EXPECT(check_pitch(9, 2, 5, "pack", "U", "dst", msg, sizeof(msg)) == nullptr);  // one side alone, as the packer asks: 4 * 2 + 1 bytes
    EXPECT(!strcmp(check_pitch(8, 2, 5, "pack", "U", "dst", msg, sizeof(msg)), "pack: plane U: dst_pitch 8 outside 9 .. 2^40"));

    // ---- n planes: a destination is exactly its source plane, or overlaps no source plane ----
    const char* const yuv[3] = {"Y", "U", "V"};
    const char* const idx[3] = {"0", "1", "2"};
    const int64_t pw[3] = {30, 15, 15}, ph[3] = {20, 10, 10};
    Plane p[3] = {plane(mem, mem, 32, 32, 1, 1), plane(mem + 1024, mem + 1024, 32, 32, 2, 2), plane(mem + 1025, mem + 1025, 32, 32, 2, 2)};  // NV12, in place
    EXPECT(!*all(p, 3, pw, ph, yuv) && !*all(p, 3, pw, ph, idx) && !*all(p, 0, pw, ph, yuv));
    // the same plane with another pitch or step is not "in place"
    p[0].dst_pitch = 40;
    EXPECT(!strcmp(all(p, 3, pw, ph, yuv), "who: plane Y: the destination starts where the source does with another pitch or step (40 and 1, not 32 and 1): in place means exactly the source plane"));
    EXPECT(!strcmp(all(p, 3, pw, ph, idx), "who: plane 0: the destination starts where the source does with another pitch or step (40 and 1, not 32 and 1): in place means exactly the source plane"));
    p[0].dst_pitch = 32, p[2].dst_step = 1;
    EXPECT(strstr(all(p, 3, pw, ph, yuv), "who: plane V: the destination starts where the source does with another pitch or step (32 and 1, not 32 and 2)") == msg);
    p[2].dst_step = 2;
    // a destination that ends exactly where a source begins is taken; one byte further it is refused.  Source plane 1 starts at mem + 1024; 10 rows of 15
    // samples, 32 and 2 bytes apart, cover 9 * 32 + 14 * 2 + 1 = 317 bytes
    p[2].dst_dev = mem + 1024 - 317;  // (source plane 0 ends at byte 19 * 32 + 30 = 638)
    EXPECT(!*all(p, 3, pw, ph, yuv));
    p[2].dst_dev = mem + 1024 - 316;
    EXPECT(!strcmp(all(p, 3, pw, ph, yuv), "who: plane V: the destination overlaps source plane U without being exactly its own source plane"));
    EXPECT(!strcmp(all(p, 3, pw, ph, idx), "who: plane 2: the destination overlaps source plane 1 without being exactly its own source plane"));
    EXPECT(!*all(p, 1, pw, ph, yuv));  // only the first n planes are looked at
    // ... and a destination that begins exactly where the last source ends (plane 2: mem + 1025 + 317)
    p[2].dst_dev = mem + 1025 + 317;
    EXPECT(!*all(p, 3, pw, ph, yuv));
    p[2].dst_dev = mem + 1025 + 316;
    EXPECT(!strcmp(all(p, 3, pw, ph, yuv), "who: plane V: the destination overlaps source plane V without being exactly its own source plane"));
    // a destination plane of another geometry: its own range counts (planar out of an interleaved source, just behind the luma plane's 638 bytes)
    p[2].dst_dev = mem + 1025;
    p[1].dst_dev = mem + 638, p[1].dst_pitch = 15, p[1].dst_step = 1;  // 150 bytes: [638, 788)
    EXPECT(!*all(p, 3, pw, ph, yuv));
    p[1].dst_dev = mem + 637;
    EXPECT(!strcmp(all(p, 3, pw, ph, yuv), "who: plane U: the destination overlaps source plane Y without being exactly its own source plane"));
    p[1].dst_dev = mem + 1024 - 150;
    EXPECT(!*all(p, 3, pw, ph, yuv));
    p[1].dst_dev = mem + 1024 - 149;
    EXPECT(!strcmp(all(p, 3, pw, ph, idx), "who: plane 1: the destination overlaps source plane 1 without being exactly its own source plane"));
    // a message that does not fit is cut, never written past the buffer the caller names (the sanitizer watches its end)
    char* small = (char*)malloc(24);
    p[0].dst_pitch = 40;
    EXPECT(check_overlap(p, 3, pw, ph, "who", yuv, small, 24) == small && strlen(small) == 23 && !strncmp(small, "who: plane Y: the desti", 23));
    free(small);
    free(mem);
    if (failures) {
        printf("%d plane_views host checks FAILED\n", failures);
        return 1;
    }
    printf("plane_views host checks passed\n");
    return 0;
}
