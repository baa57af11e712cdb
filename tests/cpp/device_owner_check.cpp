// slam-eds_amd/csrc/eds_device_owner.hpp on its own: the owner's bookkeeping against the HIP runtime, no kernel.  With a device it walks
// open / alloc / release / a refused allocation / exchanged pointers / pinned and device-mapped blocks / a regrown buffer / close / close
// again / reopen and prints "owner ok"; without one open() must answer EDS_ERR_NO_DEVICE, every kind of allocation and the regrow helper
// must refuse and leave NULL pointers and a zero capacity, close() on the owner that never opened must be harmless, and it prints
// "no device ok".
// Exit status 0 only when every check held (tests/test_device_owner.py).
#include <cstdio>
#include <string>

#include "../../slam-eds_amd/csrc/eds_device_owner.hpp"

static std::string last_message;
int edscapi::fail(int code, const std::string& msg) { last_message = msg; return code; }

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("FAILED line %d: %s\n", __LINE__, #cond); ++failures; } } while (0)

int main() {
    edscapi::DeviceOwner own;
    own.close();                                               // never opened
    CHECK(own.live() == 0 && own.st == nullptr);
    const int rc = own.open(0);
    if (rc == EDS_ERR_NO_DEVICE) {
        CHECK(last_message == "no HIP device");
        float* p = nullptr;
        CHECK(!own.alloc(p, 64) && p == nullptr && own.live() == 0);
        float *hp = nullptr, *hm = nullptr, *dm = nullptr;
        CHECK(!own.alloc_pinned(hp, 64) && hp == nullptr && own.live() == 0 && own.live_pinned() == 0);
        CHECK(!own.alloc_mapped(hm, dm, 64) && hm == nullptr && dm == nullptr && own.live() == 0 && own.live_pinned() == 0);
        size_t cap = 7;                                            // a capacity that believed in a buffer
        CHECK(!own.regrow(cap, (size_t)64, {{(void**)&p, 64}}) && p == nullptr && cap == 0);
        int slots = 3;
        CHECK(!own.regrow(slots, 8, {edscapi::mapped(hm, dm, 64), edscapi::pinned(hp, 64)}) && hm == nullptr && dm == nullptr && hp == nullptr && slots == 0);
        CHECK(own.live() == 0 && own.live_pinned() == 0);
        own.close();
        own.close();
        CHECK(own.live() == 0 && own.st == nullptr);
        std::printf(failures ? "no device: %d checks failed\n" : "no device ok\n", failures);
        return failures ? 1 : 0;
    }
    CHECK(rc == EDS_OK && own.st != nullptr);
    CHECK(own.open(1 << 20) == EDS_ERR_INVALID && last_message.rfind("device 1048576 of ", 0) == 0);

    float *a = nullptr, *c = nullptr;
    int32_t* b = nullptr;
    CHECK(own.alloc(a, 256) && a != nullptr);
    CHECK(own.alloc({{(void**)&b, 512}, {(void**)&c, 1024}}) && b != nullptr && c != nullptr);
    CHECK(own.live() == 3);
    own.release(b);
    CHECK(b == nullptr && own.live() == 2);
    own.release(b);                                            // nothing recorded under NULL
    CHECK(own.live() == 2);

    // more than any device holds: the runtime answers with an error and reserves nothing
    float* huge = nullptr;
    CHECK(!own.alloc(huge, (size_t)1 << 60) && huge == nullptr && own.live() == 2);
    CHECK(hipGetLastError() == hipSuccess);                    // alloc() cleared the runtime's error
    // ... and in a table: the entry before the refused one is freed again and every entry is NULL
    float *t0 = nullptr, *t1 = nullptr;
    CHECK(!own.alloc({{(void**)&t0, 128}, {(void**)&t1, (size_t)1 << 60}}) && t0 == nullptr && t1 == nullptr && own.live() == 2);

    // a state that did not come to life
    const size_t mark = own.live();
    float *s0 = nullptr, *s1 = nullptr;
    CHECK(own.alloc({{(void**)&s0, 128}, {(void**)&s1, 128}}) && own.live() == mark + 2);
    own.release_from(mark);
    CHECK(own.live() == mark);

    // the fields exchange their pointers (eds_winedit.hip's exchange_sets): the owner holds values, so close() frees both once
    float* t = a; a = c; c = t;
    int32_t back = 0, word = 0x5eed;
    CHECK(hipMemcpyAsync(a, &word, sizeof(word), hipMemcpyHostToDevice, own.st) == hipSuccess);
    CHECK(edscapi::read_back(own, &back, a, sizeof(back)) == EDS_OK && back == word);
    CHECK(edscapi::read_back(own, nullptr, a, sizeof(back)) == EDS_OK && edscapi::read_back(own, &back, a, 0) == EDS_OK);

    // pinned memory is a list of its own: a plain block, and a mapped pair whose host word the device reads through its own pointer
    const size_t dev_live = own.live();
    int32_t *hp = nullptr, *hm = nullptr, *dm = nullptr;
    CHECK(own.alloc_pinned(hp, 256) && hp != nullptr && own.live_pinned() == 1 && own.live() == dev_live);
    CHECK(own.alloc_mapped(hm, dm, 256) && hm != nullptr && dm != nullptr && own.live_pinned() == 2 && own.live() == dev_live);
    hm[0] = 0x0a11ce;
    back = 0;
    CHECK(hipMemcpy(&back, dm, sizeof(back), hipMemcpyDeviceToHost) == hipSuccess && back == 0x0a11ce);

    // a buffer regrown 256 -> 4096 bytes: one entry before and after, the old value gone, the new one usable
    size_t cap = 0;
    char* g = nullptr;
    CHECK(own.regrow(cap, (size_t)256, {{(void**)&g, 256}}) && g != nullptr && cap == 256);
    const size_t with_g = own.live();
    char* old = g;
    CHECK(own.regrow(cap, (size_t)4096, {{(void**)&g, 4096}}) && g != nullptr && cap == 4096 && own.live() == with_g);
    bool old_listed = false, new_listed = false;
    for (size_t i = 0; i < own.owned.n; ++i) { old_listed |= own.owned.v[i] == old && old != g; new_listed |= own.owned.v[i] == g; }
    CHECK(!old_listed && new_listed);
    CHECK(hipMemsetAsync(g, 0x5a, 4096, own.st) == hipSuccess);
    unsigned char last = 0;
    CHECK(edscapi::read_back(own, &last, g + 4095, 1) == EDS_OK && last == 0x5a);

    // pinned requests more than any host holds: alone, as a mapped pair, and through the regrow helper, which also zeroes the capacity
    const size_t pins = own.live_pinned();
    int32_t *hh = nullptr, *hd = nullptr;
    CHECK(!own.alloc_pinned(hh, (size_t)1 << 60) && hh == nullptr && own.live_pinned() == pins);
    CHECK(!own.alloc_mapped(hh, hd, (size_t)1 << 60) && hh == nullptr && hd == nullptr && own.live_pinned() == pins);
    int slots = 1;
    CHECK(!own.regrow(slots, 2, {edscapi::mapped(hm, dm, (size_t)1 << 60)}) && hm == nullptr && dm == nullptr && slots == 0);
    CHECK(own.live_pinned() == pins - 1 && own.live() == with_g);            // the pair that was to grow is gone, nothing else
    CHECK(hipGetLastError() == hipSuccess);
    // a mixed table refused at its last entry: what came before is freed from both lists
    CHECK(!own.alloc({edscapi::pinned(hh, 64), {(void**)&t0, 64}, edscapi::mapped(hm, dm, (size_t)1 << 60)}) && hh == nullptr && t0 == nullptr &&
          hm == nullptr && dm == nullptr && own.live_pinned() == pins - 1 && own.live() == with_g);
    own.release(hp);
    CHECK(hp == nullptr && own.live_pinned() == pins - 2);
    CHECK(own.alloc_pinned(hp, 64) && own.live_pinned() == pins - 1);       // left for close()

    own.close();
    CHECK(own.live() == 0 && own.live_pinned() == 0 && own.st == nullptr);
    own.close();
    CHECK(own.live() == 0 && own.live_pinned() == 0);

    CHECK(own.open(0) == EDS_OK && own.alloc(a, 256) && own.live() == 1);
    own.close();
    CHECK(own.live() == 0);
    std::printf(failures ? "owner: %d checks failed\n" : "owner ok\n", failures);
    return failures ? 1 : 0;
}
