// multiseq_longctx_test.cpp — the multi-sequence and the long-context option of the
// ggml-backend registration together (ggml_backend_mi355x_set_multi_seq, _set_long_context,
// adapter/ggml-mi355x.cpp), driven like multiseq_test.cpp: reg -> device -> init_backend ->
// buffer -> set_tensor -> graph_compute -> get_tensor. Test infrastructure
// (tests/test_gpu_adapter_multiseq_stream.py), compiled with -Werror against the restated ggml
// headers in tests/adapter/ggml/ and ggml_stub.cpp.
//
//   multiseq_longctx_test graph.txt blob.bin tokens.txt out.bin buffer_bytes n_vocab on|off positions
//       The files are glue_test decode's, for a decode graph over a cache past the attention
//       kernels' LDS sizes; positions: one per token of tokens.txt, comma-separated, each >= 2.
//       Token i is decoded at cell == position positions[i] with cell 1 hidden by the mask — a
//       graph the cells == positions promise does not cover, so with the multi-sequence option
//       (always on here) it runs as ATTN_BATCH nodes. With long-context "on" (both options set
//       through the registry's get_proc_address) every step must succeed and its logits go to
//       out.bin; with "off" (the default) the first step must be refused ("refused -1").
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "ggml-backend-impl.h"
#include "ggml-mi355x.h"
#include "ggml_mi355x.h"
#include "ggml_stub.h"

static const uint64_t BASE = 1ull << 44;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);         \
            return 1;                                                       \
        }                                                                   \
    } while (0)

struct Loaded {
    std::vector<ggml_tensor *> all, nodes;
    std::unordered_map<std::string, ggml_tensor *> by_name;
};

// the serialization of tests/test_adapter.py (one "T" line per tensor, one "N" line of node ids)
static bool load_graph(const char *path, Loaded &L, char *base) {
    std::ifstream in(path);
    std::unordered_map<long, ggml_tensor *> byid;
    std::vector<std::vector<long>> refs;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string tag;
        s >> tag;
        if (tag == "T") {
            auto *t = new ggml_tensor();
            long id;
            int type;
            std::string opn, name;
            s >> id >> type >> opn;
            t->type = (ggml_type)type;
            t->op = stub_op_of_name(opn.c_str());
            if (t->op == GGML_OP_COUNT) return false;
            for (auto &v : t->ne) s >> v;
            for (auto &v : t->nb) s >> v;
            for (auto &v : t->op_params) s >> v;
            s >> t->flags;
            std::vector<long> r(GGML_MAX_SRC + 1);
            for (auto &v : r) s >> v;
            unsigned long long data;
            s >> t->view_offs >> data >> name;
            t->data = data >= BASE ? (void *)(base + (data - BASE)) : (void *)(uintptr_t)data;
            if (name != "-") std::strncpy(t->name, name.c_str(), GGML_MAX_NAME - 1);
            if (!L.by_name.count(t->name)) L.by_name[t->name] = t;
            byid[id] = t;
            L.all.push_back(t);
            refs.push_back(r);
        } else if (tag == "N") {
            int n;
            s >> n;
            for (int i = 0; i < n; ++i) {
                long id;
                s >> id;
                L.nodes.push_back(byid.at(id));
            }
        }
    }
    for (size_t i = 0; i < L.all.size(); ++i) {
        for (int j = 0; j < GGML_MAX_SRC; ++j) L.all[i]->src[j] = refs[i][j] >= 0 ? byid.at(refs[i][j]) : nullptr;
        L.all[i]->view_src = refs[i][GGML_MAX_SRC] >= 0 ? byid.at(refs[i][GGML_MAX_SRC]) : nullptr;
    }
    return !L.nodes.empty();
}

typedef void (*set_multi_seq_fn)(ggml_backend_t, bool);
typedef void (*set_long_context_fn)(bool);

int main(int argc, char **argv) {
    if (argc < 9) return 2;
    const size_t buf_bytes = std::strtoull(argv[5], nullptr, 0);
    const int64_t n_vocab = std::atoll(argv[6]);
    const bool on = std::strcmp(argv[7], "on") == 0;
    std::vector<int> positions;
    {
        std::istringstream ps(argv[8]);
        std::string item;
        while (std::getline(ps, item, ',')) positions.push_back(std::atoi(item.c_str()));
    }
    ggml_backend_reg_t reg = ggml_backend_mi355x_reg();
    CHECK(reg->iface.get_device_count(reg) >= 1);
    auto set_multi_seq = (set_multi_seq_fn)reg->iface.get_proc_address(reg, "ggml_backend_mi355x_set_multi_seq");
    CHECK(set_multi_seq == ggml_backend_mi355x_set_multi_seq);
    auto set_long_context = (set_long_context_fn)reg->iface.get_proc_address(reg, "ggml_backend_mi355x_set_long_context");
    CHECK(set_long_context == ggml_backend_mi355x_set_long_context);
    ggml_backend_dev_t dev = reg->iface.get_device(reg, 0);
    ggml_backend_t be = dev->iface.init_backend(dev, nullptr);
    CHECK(be != nullptr);
    set_multi_seq(be, true);
    if (on) set_long_context(true);  // the default is off
    ggml_backend_buffer_type_t buft = dev->iface.get_buffer_type(dev);
    ggml_backend_buffer_t buf = buft->iface.alloc_buffer(buft, buf_bytes);
    CHECK(buf && buf->size == buf_bytes);
    char *base = (char *)buf->iface.get_base(buf);
    buf->iface.clear(buf, 0);

    Loaded L;
    CHECK(load_graph(argv[1], L, base));
    for (ggml_tensor *t : L.all)
        if ((char *)t->data >= base && (char *)t->data < base + buf_bytes) t->buffer = buf;
    {
        std::ifstream bin(argv[2], std::ios::binary);
        ggml_tensor whole{};
        whole.data = base;
        whole.buffer = buf;
        uint64_t hdr[2];
        std::vector<char> bytes;
        while (bin.read((char *)hdr, sizeof(hdr))) {
            bytes.resize(hdr[1]);
            bin.read(bytes.data(), (std::streamsize)hdr[1]);
            CHECK(hdr[0] + hdr[1] <= buf_bytes);
            buf->iface.set_tensor(buf, &whole, bytes.data(), hdr[0], hdr[1]);
        }
    }
    ggml_tensor *tok = L.by_name.at("inp_tokens"), *pos = L.by_name.at("inp_pos"), *mask = L.by_name.at("kq_mask");
    ggml_tensor *kid = L.by_name.at("k_idxs"), *vid = L.by_name.at("v_idxs");
    ggml_tensor *logits = L.nodes.back();
    CHECK(logits->ne[0] == n_vocab && (logits->flags & GGML_TENSOR_FLAG_OUTPUT));
    const int64_t n_kv = mask->ne[0];
    ggml_cgraph *cg = stub_graph_new(L.nodes.data(), (int)L.nodes.size());
    std::vector<int32_t> tokens;
    {
        std::ifstream tin(argv[3]);
        int32_t v;
        while (tin >> v) tokens.push_back(v);
    }
    CHECK(!tokens.empty() && tokens.size() == positions.size());
    for (int p : positions) CHECK(p >= 2 && p < n_kv);
    auto set_inputs = [&](int p, int32_t token, int hide_cell) {
        const int32_t tp[1] = {token}, pp[1] = {p};
        buf->iface.set_tensor(buf, tok, tp, 0, 4);
        buf->iface.set_tensor(buf, pos, pp, 0, 4);
        const int64_t kk[1] = {p};
        buf->iface.set_tensor(buf, kid, kk, 0, 8);
        std::vector<int64_t> vv((size_t)ggml_nelements(vid));
        for (size_t i = 0; i < vv.size(); ++i) vv[i] = (int64_t)i * n_kv + p;
        buf->iface.set_tensor(buf, vid, vv.data(), 0, vv.size() * 8);
        std::vector<uint8_t> m((size_t)mask->nb[1]);
        for (int64_t j = 0; j < n_kv; ++j) {
            const bool vis = j <= p && j != hide_cell;
            if (mask->type == GGML_TYPE_F16) {
                const uint16_t h = vis ? 0 : 0xfc00;
                std::memcpy(m.data() + 2 * j, &h, 2);
            } else {
                const float f = vis ? 0.f : -INFINITY;
                std::memcpy(m.data() + 4 * j, &f, 4);
            }
        }
        buf->iface.set_tensor(buf, mask, m.data(), 0, m.size());
    };
    FILE *out = std::fopen(argv[4], "wb");
    CHECK(out != nullptr);
    std::vector<float> lg((size_t)n_vocab);
    // every step a hidden-cell graph: cell 1 (another sequence's, or a removed one) inside [0, pos]
    for (size_t i = 0; i < tokens.size(); ++i) {
        set_inputs(positions[i], tokens[i], 1);
        const ggml_status st = be->iface.graph_compute(be, cg);
        be->iface.synchronize(be);
        if (!on) {
            std::printf("refused %d\n", (int)st);
            CHECK(st == GGML_STATUS_FAILED);
            break;
        }
        std::printf("hidden %zu pos %d status %d\n", i, positions[i], (int)st);
        CHECK(st == GGML_STATUS_SUCCESS);
        buf->iface.get_tensor(buf, logits, lg.data(), 0, lg.size() * 4);
        std::fwrite(lg.data(), 4, lg.size(), out);
    }
    std::fclose(out);
    stub_graph_free(cg);
    buf->iface.free_buffer(buf);
    delete buf;
    be->iface.free(be);
    for (ggml_tensor *t : L.all) delete t;
    std::printf("ok\n");
    return 0;
}
