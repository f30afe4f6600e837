// jxg_djxl -- djxl-argv-compatible decoder over the C ABI: the counterpart of
// jxg_cjxl for the harness's decode step (the legacy old_test_jxl.py shells
// out to `djxl IN.jxl OUT.png`).
//
//   jxg_djxl IN.jxl OUT.{ppm,png} [--device=N]
//   jxg_djxl --batch=LIST [--device=N]
//
// LIST holds one IN<TAB>OUT per line: all files go through one context and one
// jxg_decode_batch_rgb8 call, so HIP starts once per list instead of once per
// file and the frames share the pass-group launches.  Every failed file is one
// stderr line (IN: status, or the I/O error); the others are still written;
// exit 0 only if every file was written.
//
// .ppm writes a binary P6, .png an 8-bit RGB PNG (filter type 0, zlib level 1;
// csrc/jxg_cli_io.h has the writer beside the reader jxg_cjxl uses).  Exit 0 on success; on failure
// exit 1 with one line on stderr: jxg_status_str of the status, or the I/O
// error.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/jxg.h"
#include "jxg_cli_io.h"

namespace {

using namespace jxg_cli;

bool ends_with(const std::string& s, const char* suffix) {
  const size_t n = std::strlen(suffix);
  if (s.size() < n) return false;
  for (size_t i = 0; i < n; i++) {
    char c = s[s.size() - n + i];
    if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
    if (c != suffix[i]) return false;
  }
  return true;
}

// one line on stderr and false when the image cannot be written
bool write_image(const char* path, bool png, const std::vector<uint8_t>& rgb, uint32_t w, uint32_t h) {
  std::vector<uint8_t> file;
  if (png && !encode_png(rgb, w, h, file)) {
    std::fprintf(stderr, "PNG deflate failed\n");
    return false;
  }
  if (!(png ? write_file(path, file.data(), file.size()) : write_ppm(path, rgb.data(), w, h))) {
    std::fprintf(stderr, "cannot write %s\n", path);
    return false;
  }
  return true;
}

jxg_ctx* create_ctx(int device) {
  jxg_params p{};
  p.distance = 1.0f;
  p.effort = 7;
  p.num_devices = 1;
  p.device = device;
  jxg_ctx* ctx = nullptr;
  const jxg_status st = jxg_create(&p, &ctx);
  if (st != JXG_OK) {
    std::fprintf(stderr, "jxg_create: %s\n", jxg_status_str(st));
    return nullptr;
  }
  return ctx;
}

struct Item {  // one IN<TAB>OUT line of a batch list
  std::string in, out;
  bool png = false, ok = false;
  std::vector<uint8_t> data, rgb;
  jxg_stream_info info{};
};

// the list's lines; one line on stderr and false for a list that cannot be run
bool read_batch_list(const char* list_path, std::vector<Item>& items) {
  std::vector<uint8_t> list;
  if (!read_file(list_path, list)) {
    std::fprintf(stderr, "cannot read %s\n", list_path);
    return false;
  }
  const std::string text(list.begin(), list.end());
  for (size_t at = 0; at < text.size();) {
    size_t nl = text.find('\n', at);
    if (nl == std::string::npos) nl = text.size();
    std::string line = text.substr(at, nl - at);
    at = nl + 1;
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    const size_t tab = line.find('\t');
    if (tab == std::string::npos || tab == 0 || tab + 1 == line.size()) {
      std::fprintf(stderr, "%s: a line is not IN<TAB>OUT\n", list_path);
      return false;
    }
    Item it;
    it.in = line.substr(0, tab);
    it.out = line.substr(tab + 1);
    items.push_back(std::move(it));
  }
  if (items.empty()) std::fprintf(stderr, "%s: no files listed\n", list_path);
  return !items.empty();
}

// --batch=LIST: every IN<TAB>OUT line of the list through one context and one
// jxg_decode_batch_rgb8 call; a failed file is one stderr line, the others are
// still written.  0 only if every file was written.
int run_batch(const char* list_path, int device) {
  std::vector<Item> items;
  if (!read_batch_list(list_path, items)) return 1;
  // the files the call can take: readable, a codestream, a known output type
  std::vector<Item*> sent;
  for (Item& it : items) {
    it.png = ends_with(it.out, ".png");
    if (!it.png && !ends_with(it.out, ".ppm")) {
      std::fprintf(stderr, "%s: output must be .ppm or .png\n", it.out.c_str());
      continue;
    }
    if (!read_file(it.in.c_str(), it.data)) {
      std::fprintf(stderr, "cannot read %s\n", it.in.c_str());
      continue;
    }
    const jxg_status st = it.data.empty()
                              ? JXG_ERR_INVALID_ARG
                              : jxg_decode_info(it.data.data(), it.data.size(), &it.info);
    if (st != JXG_OK) {
      std::fprintf(stderr, "%s: %s\n", it.in.c_str(), jxg_status_str(st));
      continue;
    }
    it.rgb.resize((size_t)it.info.xsize * it.info.ysize * 3);
    sent.push_back(&it);
  }
  if (!sent.empty()) {
    jxg_ctx* ctx = create_ctx(device);
    if (!ctx) return 1;
    const uint32_t n = (uint32_t)sent.size();
    std::vector<const uint8_t*> datas(n);
    std::vector<size_t> sizes(n), strides(n);
    std::vector<uint8_t*> rgbs(n);
    std::vector<jxg_status> st(n, JXG_OK);
    for (uint32_t i = 0; i < n; i++) {
      datas[i] = sent[i]->data.data();
      sizes[i] = sent[i]->data.size();
      rgbs[i] = sent[i]->rgb.data();
      strides[i] = (size_t)sent[i]->info.xsize * 3;
    }
    const jxg_status call = jxg_decode_batch_rgb8(ctx, datas.data(), sizes.data(), n, rgbs.data(),
                                                  strides.data(), st.data());
    jxg_destroy(ctx);
    // a call refused outright writes no statuses: every file has the call's
    bool any = false;
    for (uint32_t i = 0; i < n; i++) any = any || st[i] != JXG_OK;
    for (uint32_t i = 0; i < n; i++) {
      const jxg_status s = call != JXG_OK && !any ? call : st[i];
      if (s != JXG_OK) {
        std::fprintf(stderr, "%s: %s\n", sent[i]->in.c_str(), jxg_status_str(s));
        continue;
      }
      sent[i]->ok = write_image(sent[i]->out.c_str(), sent[i]->png, sent[i]->rgb,
                                sent[i]->info.xsize, sent[i]->info.ysize);
    }
  }
  for (const Item& it : items)
    if (!it.ok) return 1;
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  int device = 0;
  const char* batch = nullptr;
  std::vector<const char*> pos;
  for (int i = 1; i < argc; i++) {
    if (!std::strncmp(argv[i], "--device=", 9))
      device = std::atoi(argv[i] + 9);
    else if (!std::strncmp(argv[i], "--batch=", 8))
      batch = argv[i] + 8;
    else if (!std::strncmp(argv[i], "--", 2))
      continue;  // djxl options that do not change the pixels of an 8-bit decode
    else
      pos.push_back(argv[i]);
  }
  if (batch && pos.empty()) return run_batch(batch, device);
  if (batch || pos.size() != 2) {
    std::fprintf(stderr,
                 "usage: jxg_djxl IN.jxl OUT.{ppm,png} [--device=N]\n"
                 "       jxg_djxl --batch=LIST [--device=N]   (LIST: one IN<TAB>OUT per line)\n");
    return 1;
  }
  const std::string out_path = pos[1];
  const bool png = ends_with(out_path, ".png");
  if (!png && !ends_with(out_path, ".ppm")) {
    std::fprintf(stderr, "%s: output must be .ppm or .png\n", pos[1]);
    return 1;
  }
  std::vector<uint8_t> data;
  if (!read_file(pos[0], data)) {
    std::fprintf(stderr, "cannot read %s\n", pos[0]);
    return 1;
  }
  jxg_stream_info info{};
  jxg_status st = data.empty() ? JXG_ERR_INVALID_ARG : jxg_decode_info(data.data(), data.size(), &info);
  if (st != JXG_OK) {
    std::fprintf(stderr, "%s: %s\n", pos[0], jxg_status_str(st));
    return 1;
  }
  jxg_ctx* ctx = create_ctx(device);
  if (!ctx) return 1;
  std::vector<uint8_t> rgb((size_t)info.xsize * info.ysize * 3);
  st = jxg_decode_rgb8(ctx, data.data(), data.size(), rgb.data(), (size_t)info.xsize * 3);
  jxg_destroy(ctx);
  if (st != JXG_OK) {
    std::fprintf(stderr, "%s: %s\n", pos[0], jxg_status_str(st));
    return 1;
  }
  return write_image(pos[1], png, rgb, info.xsize, info.ysize) ? 0 : 1;
}
