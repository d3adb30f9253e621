// The planner's time-allocation network (network/utils/learning/minsnap_network_conv_lstm.py:37-88, 114-187) behind
// anet_timenet_*: the replacement of the torch::jit::script::Module member of LearningPlanner and of its forward call.
// No libtorch: the weights come from the flat file the Python package writes (allocnet_amd.TimeAllocNet.save):
//   8 bytes "ANETTIME", uint32 version (1), uint32 seq_len, uint32 hidden, then the 16 tensors of the state dict as
//   little-endian float32 in the order of allocnet_amd.h (anet_timenet_create), natural shapes.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "core.hpp"

namespace anet {

class TimeAllocNet {
 public:
  TimeAllocNet() = default;
  ~TimeAllocNet() { reset(); }
  TimeAllocNet(const TimeAllocNet &) = delete;
  TimeAllocNet &operator=(const TimeAllocNet &) = delete;

  bool loaded() const { return net_ != nullptr; }
  int seq_len() const { return seq_len_; }
  int hidden() const { return hidden_; }

  // Reads the weights file and uploads it.  Throws anet::Error on a malformed file or a model the kernels do not take.
  void load(const std::string &path) {
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) throw Error(ANET_ERR_INVALID, "TimeAllocNet::load: cannot open " + path);
    std::vector<unsigned char> buf;
    unsigned char chunk[65536];
    size_t got;
    while ((got = std::fread(chunk, 1, sizeof(chunk), f)) > 0) buf.insert(buf.end(), chunk, chunk + got);
    std::fclose(f);
    if (buf.size() < 20 || std::memcmp(buf.data(), "ANETTIME", 8) != 0)
      throw Error(ANET_ERR_INVALID, "TimeAllocNet::load: " + path + " is not a time-allocation weights file");
    const uint32_t version = le32(&buf[8]), seq = le32(&buf[12]), hid = le32(&buf[16]);
    if (version != 1 || (seq != 5 && seq != 10) || hid < 1 || hid > 4096)
      throw Error(ANET_ERR_UNSUPPORTED, "TimeAllocNet::load: version, seq_len or hidden not supported");
    const size_t H = hid, flat = 16 * (size_t)(seq / 4);
    const size_t n[ANET_TIMENET_TENSORS] = {8 * 9 * 3, 8, 6 * 8, 6, 16 * 50 * 9, 16, 32 * flat, 32, 4 * H * 38, 4 * H * H,
                                            4 * H,     4 * H, H, 1, H, 1};
    size_t total = 0;
    for (size_t k : n) total += k;
    if (buf.size() != 20 + 4 * total) throw Error(ANET_ERR_INVALID, "TimeAllocNet::load: the header announces another size");
    std::vector<float> w(total);
    for (size_t i = 0; i < total; ++i) {
      const uint32_t bits = le32(&buf[20 + 4 * i]);
      std::memcpy(&w[i], &bits, 4);
    }
    const float *ptrs[ANET_TIMENET_TENSORS];
    size_t off = 0;
    for (int i = 0; i < ANET_TIMENET_TENSORS; ++i) {
      ptrs[i] = w.data() + off;
      off += n[i];
    }
    Context &ctx = Context::thread_default();
    anet_timenet *net = nullptr;
    ctx.check(anet_timenet_create(ctx.get(), (int)seq, (int)hid, ptrs, &net));
    reset();
    net_ = net;
    seq_len_ = (int)seq;
    hidden_ = (int)hid;
  }

  // state [batch][9][2], hpolys [batch][50][4][seq_len]; times [batch][seq_len], count [batch]; tf, stop may be nullptr
  void forward(int64_t batch, const float *state, const float *hpolys, double threshold, float *times, int32_t *count,
               float *tf = nullptr, float *stop = nullptr, int flags = 0) const {
    if (!net_) throw Error(ANET_ERR_INVALID, "TimeAllocNet::forward before load");
    Context &ctx = Context::thread_default();
    ctx.check(anet_timenet_forward(ctx.get(), net_, seq_len_, batch, state, hpolys, threshold, flags, times, tf, stop, count));
  }

 private:
  static uint32_t le32(const unsigned char *p) {
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
  }
  void reset() {
    if (net_) anet_timenet_destroy(net_);
    net_ = nullptr;
  }
  anet_timenet *net_ = nullptr;
  int seq_len_ = 0, hidden_ = 0;
};

}  // namespace anet
