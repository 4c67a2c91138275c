// fe_host_sanitize.cpp -- the host half of the whole-frame feature tracker (is-vins_amd/csrc/isv_fe_host.h) stand-alone under
// AddressSanitizer + UBSan (tests/test_fe_sanitize.py builds and runs it): the item checks, the refusal of slots named twice, the
// validation of a planted state and PubImageData's gate, each on good and on hostile inputs.  Every array is heap-allocated at its
// exact size, so that a read past a count is a report.  No GPU, nothing loaded into Python.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <vector>
#include "../../is-vins_amd/csrc/isv_fe_host.h"

#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            return 1;                                                   \
        }                                                               \
    } while (0)

static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

struct Planted {                  // a state of n points, every array exactly n long
    isv_fe_state_t st{};
    std::unique_ptr<float[]> pts, un;
    std::unique_ptr<int32_t[]> ids, cnt;
    std::unique_ptr<uint8_t[]> map;
    explicit Planted(int n, int alloc = -1) {
        const int a = alloc < 0 ? n : alloc;
        pts.reset(new float[2 * a]); un.reset(new float[2 * a]); ids.reset(new int32_t[a]); cnt.reset(new int32_t[a]); map.reset(new uint8_t[a]);
        for (int i = 0; i < a; i++) {
            pts[2 * i] = 1.f + (float)(i % 150); pts[2 * i + 1] = 2.f + (float)(i % 100);
            un[2 * i] = 0.01f * i; un[2 * i + 1] = -0.01f * i;
            ids[i] = i; cnt[i] = 1 + i % 7; map[i] = (uint8_t)(i & 1);
        }
        st.has_sequence = 1; st.n_points = n; st.n_id = a; st.prev_time = 1.5;
    }
    int check(int max_points, const FeSlotView &v) const { return fe_check_state(max_points, v, &st, pts.get(), ids.get(), cnt.get(), un.get(), map.get()); }
};

int main() {
    int checks = 0;
    // ---- the item checks ----
    std::vector<uint8_t> img(160 * 120);
    isv_fe_item_t good{3, 160, 120, 160, img.data(), 0.25, 1, 0};
    CHECK(fe_check_item(8, 160, 120, &good, 1) == ISV_TRK_OK);
    struct { int32_t slot, w, h, stride; bool null_cur; double t; int have; int want; } bad[] = {
        {3, 0, 120, 160, false, 0.0, 1, ISV_TRK_INPUT},   {3, 160, -1, 160, false, 0.0, 1, ISV_TRK_INPUT},  {3, 160, 120, 159, false, 0.0, 1, ISV_TRK_INPUT},
        {-1, 160, 120, 160, false, 0.0, 1, ISV_TRK_INPUT}, {8, 160, 120, 160, false, 0.0, 1, ISV_TRK_INPUT}, {INT32_MAX, 160, 120, 160, false, 0.0, 1, ISV_TRK_INPUT},
        {3, 160, 120, 160, true, 0.0, 1, ISV_TRK_INPUT},  {3, 160, 120, 160, false, 0.0, 0, ISV_TRK_INPUT},  {3, 160, 120, 160, false, kNaN, 1, ISV_TRK_INPUT},
        {3, 160, 120, 160, false, kInf, 1, ISV_TRK_INPUT}, {3, 160, 120, 160, false, -kInf, 1, ISV_TRK_INPUT}, {3, 161, 120, 161, false, 0.0, 1, ISV_TRK_CAPACITY},
        {3, 160, 121, 160, false, 0.0, 1, ISV_TRK_CAPACITY}, {3, INT32_MAX, INT32_MAX, INT32_MAX, false, 0.0, 1, ISV_TRK_CAPACITY}, {3, 160, 120, INT32_MIN, false, 0.0, 1, ISV_TRK_INPUT}};
    for (const auto &b : bad) {
        isv_fe_item_t it{b.slot, b.w, b.h, b.stride, b.null_cur ? nullptr : img.data(), b.t, 1, 0};
        CHECK(fe_check_item(8, 160, 120, &it, b.have) == b.want);
        checks++;
    }
    // ---- the slot's checks ----
    const FeSlotView none{0, 0, 0, 1, 0, 0}, fresh{1, 160, 120, 1, 1, 1};
    CHECK(fe_check_slot(&good, none) == ISV_TRK_OK);              // a first frame takes any slot
    CHECK(fe_check_slot(&good, fresh) == ISV_TRK_OK);
    for (FeSlotView v : {FeSlotView{0, 160, 120, 1, 1, 1}, FeSlotView{1, 160, 120, 0, 1, 1}, FeSlotView{1, 160, 120, 1, 1, 0}, FeSlotView{1, 161, 120, 1, 1, 1},
                         FeSlotView{1, 160, 119, 1, 1, 1}}) {
        CHECK(fe_check_slot(&good, v) == ISV_TRK_INPUT);          // no image, another writer's tag, a replaced image, another size
        checks++;
    }
    // ---- slots named twice ----
    {
        const int n = 9;
        std::unique_ptr<int32_t[]> slot(new int32_t[n]{5, 2, 5, 7, 2, 9, 5, 1, 7}), st(new int32_t[n]{0, 0, 0, 2, 0, 0, 1, 0, 0});
        fe_refuse_duplicates(n, slot.get(), st.get());
        const int32_t want[n] = {2, 2, 2, 2, 2, 0, 1, 0, 0};      // 5 and 2 twice among the good ones; the refused 7 and 5 do not count
        for (int i = 0; i < n; i++) CHECK(st[i] == want[i]);
        fe_refuse_duplicates(0, slot.get(), st.get());
        std::vector<int32_t> many(4096), ok(4096, 0);
        for (int i = 0; i < 4096; i++) many[i] = i / 2;
        fe_refuse_duplicates(4096, many.data(), ok.data());
        for (int i = 0; i < 4096; i++) CHECK(ok[i] == ISV_TRK_INPUT);
        checks += 3;
    }
    // ---- the planted state ----
    const FeSlotView slot{1, 160, 120, 1, 0, 0};
    for (int n : {0, 1, 7, 64, 65, 129, 160}) {
        CHECK(Planted(n).check(160, slot) == ISV_OK);
        checks++;
    }
    {
        Planted none_needed(0);
        CHECK(fe_check_state(160, slot, &none_needed.st, nullptr, nullptr, nullptr, nullptr, nullptr) == ISV_OK);      // no point, no array
        Planted p(161);
        CHECK(p.check(160, slot) == ISV_ERR_CAPACITY);
        Planted big(4, 4);
        big.st.n_points = INT32_MAX;                               // a count far beyond the arrays: refused before anything is read
        CHECK(big.check(160, slot) == ISV_ERR_CAPACITY);
        big.st.n_points = -1;
        CHECK(big.check(160, slot) == ISV_ERR_INVALID_ARG);
        big.st.n_points = INT32_MIN;
        CHECK(big.check(160, slot) == ISV_ERR_INVALID_ARG);
        Planted q(8);
        CHECK(fe_check_state(160, slot, &q.st, q.pts.get(), nullptr, q.cnt.get(), q.un.get(), q.map.get()) == ISV_ERR_INVALID_ARG);
        CHECK(q.check(160, FeSlotView{0, 160, 120, 1, 0, 0}) == ISV_ERR_INVALID_ARG);      // no resident image
        CHECK(q.check(160, FeSlotView{1, 160, 120, 0, 0, 0}) == ISV_ERR_INVALID_ARG);      // another writer's image
        checks += 8;
    }
    {
        auto spoil = [&](auto &&f) {
            Planted p(12);
            f(p);
            return p.check(160, slot);
        };
        const float fnan = std::numeric_limits<float>::quiet_NaN(), finf = std::numeric_limits<float>::infinity();
        CHECK(spoil([&](Planted &p) { p.pts[5] = fnan; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.pts[4] = -finf; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.pts[4] = 3e38f; }) == ISV_ERR_INVALID_ARG);        // beyond int: rounds to nothing
        CHECK(spoil([&](Planted &p) { p.pts[4] = -0.51f; }) == ISV_ERR_INVALID_ARG);       // rounds to -1
        CHECK(spoil([&](Planted &p) { p.pts[4] = -0.5f; }) == ISV_OK);                     // half to even: 0
        CHECK(spoil([&](Planted &p) { p.pts[4] = 159.5f; }) == ISV_ERR_INVALID_ARG);       // half to even: 160
        CHECK(spoil([&](Planted &p) { p.pts[4] = 159.49f; }) == ISV_OK);
        CHECK(spoil([&](Planted &p) { p.pts[5] = 119.51f; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.un[7] = fnan; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.ids[3] = p.ids[9]; }) == ISV_ERR_INVALID_ARG);     // twice
        CHECK(spoil([&](Planted &p) { p.ids[3] = -1; p.ids[9] = -1; }) == ISV_OK);         // -1 may repeat
        CHECK(spoil([&](Planted &p) { p.ids[3] = -2; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.ids[3] = 12; }) == ISV_ERR_INVALID_ARG);           // not below n_id
        CHECK(spoil([&](Planted &p) { p.ids[3] = INT32_MAX; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.st.n_id = -1; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.cnt[0] = 0; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.cnt[0] = INT32_MAX; }) == ISV_ERR_INVALID_ARG);    // track_cnt++ would overflow
        CHECK(spoil([&](Planted &p) { p.cnt[0] = 1 << 30; }) == ISV_OK);
        CHECK(spoil([&](Planted &p) { p.map[11] = 2; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.st.prev_time = kNaN; }) == ISV_ERR_INVALID_ARG);
        CHECK(spoil([&](Planted &p) { p.st.prev_time = -kInf; }) == ISV_ERR_INVALID_ARG);
        checks += 21;
    }
    // ---- the gate ----
    {
        isv_fe_gate_t g;
        isv_fe_gate_out_t o;
        CHECK(fe_gate_init(nullptr, 10) == ISV_ERR_INVALID_ARG && fe_gate_init(&g, 0) == ISV_ERR_INVALID_ARG && fe_gate_init(&g, INT32_MIN) == ISV_ERR_INVALID_ARG);
        CHECK(fe_gate_init(&g, 10) == ISV_OK && g.pub_count == 1 && g.first_image_flag == 1 && g.init_feature == 0 && g.init_pub == 0);
        CHECK(fe_gate_step(nullptr, 0.0, &o) == ISV_ERR_INVALID_ARG && fe_gate_step(&g, 0.0, nullptr) == ISV_ERR_INVALID_ARG);
        int published = 0, delivered = 0;
        for (int i = 0; i < 400; i++) {                           // 20 s at 20 Hz: every other frame, the first message dropped
            CHECK(fe_gate_step(&g, 100.0 + 0.05 * i, &o) == ISV_OK);
            published += o.pub_this_frame; delivered += o.deliver;
            CHECK(!o.skip || (!o.pub_this_frame && !o.deliver));
        }
        CHECK(published >= 195 && published <= 200 && delivered == published - 1);
        // hostile stamps: none may trap, overflow an integer or publish on nonsense
        CHECK(fe_gate_init(&g, INT32_MAX) == ISV_OK);
        const double hostile[] = {0.0, 0.0, 0.0, kNaN, 1.0, kInf, -kInf, 1e308, -1e308, 5e-324, 1.0, 1.0, 1.0 + 1e-16, kNaN, kNaN, 2.0, 2.5, 2.5, 3.0};
        for (double t : hostile) {
            CHECK(fe_gate_step(&g, t, &o) == ISV_OK);
            CHECK((o.skip == 0 || o.skip == 1) && (o.pub_this_frame == 0 || o.pub_this_frame == 1) && g.pub_count >= 0);
        }
        g.pub_count = INT32_MAX; g.first_image_flag = 0; g.init_feature = 1; g.first_image_time = 0.0; g.last_image_time = 1.0; g.freq = INT32_MAX;
        CHECK(fe_gate_step(&g, 1.5, &o) == ISV_OK && g.pub_count == INT32_MAX);           // the count saturates
        g.freq = 0;
        CHECK(fe_gate_step(&g, 1.6, &o) == ISV_ERR_INVALID_ARG);
        checks += 6;
    }
    printf("ok: %d groups of checks on the front end's host half\n", checks);
    return 0;
}
