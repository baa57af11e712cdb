// slam-eds_amd/csrc/eds_device_owner.hpp on its own: the owner's bookkeeping against the HIP runtime, no kernel.  With a device it walks
// open / alloc / release / a refused allocation / exchanged pointers / close / close again / reopen and prints "owner ok"; without one
// open() must answer EDS_ERR_NO_DEVICE and close() on the owner that never opened must be harmless, and it prints "no device ok".
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

    own.close();
    CHECK(own.live() == 0 && own.st == nullptr);
    own.close();
    CHECK(own.live() == 0);

    CHECK(own.open(0) == EDS_OK && own.alloc(a, 256) && own.live() == 1);
    own.close();
    CHECK(own.live() == 0);
    std::printf(failures ? "owner: %d checks failed\n" : "owner ok\n", failures);
    return failures ? 1 : 0;
}
