// image_io.cpp — the canvas writers of the reference (canvas.rs:75-137) for
// the 8-bit frames the device produces (RT_OUT_U8: canvas.rs:117-123's
// quantization happens in the kernel's store).  Host I/O, off the timed path:
//   Canvas::to_ppm_file   canvas.rs:75-97, 107-112 -> the same P3 text, byte
//                                              for byte: header lines "P3",
//                                              "W H", "255"; then 5 pixels (15
//                                              channels) per line whatever the
//                                              row boundaries, each channel
//                                              right-aligned to width 3 and
//                                              joined by single spaces; lines
//                                              joined by '\n', no trailing
//                                              newline.  A binary P6 is an
//                                              explicit opt-in
//                                              (RT_IMAGE_PPM_BINARY).
//   Canvas::to_png_file   canvas.rs:114-137 -> RGB8 PNG, filter None on every
//                                              row, deflate at the highest
//                                              level (image's
//                                              CompressionType::Best,
//                                              FilterType::NoFilter)
//   Canvas::prepare_file  canvas.rs:99-105  -> the parent directories are
//                                              created first (create_dir_all)
//   Color::clamped + the u8 cast  canvas.rs:81, 117-123 -> rt_canvas_quantize
//                                              for f64 canvases on the host
#include <zlib.h>

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "../../include/rtc_scene.h"
#include "rtc_internal.hpp"

namespace {

void put_be32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24));
    v.push_back((uint8_t)(x >> 16));
    v.push_back((uint8_t)(x >> 8));
    v.push_back((uint8_t)x);
}

// One PNG chunk: length, type, data, CRC-32 of type + data.
void chunk(std::vector<uint8_t>& out, const char type[4], const uint8_t* data, size_t n) {
    put_be32(out, (uint32_t)n);
    const size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    if (n) out.insert(out.end(), data, data + n);
    put_be32(out, (uint32_t)crc32(0L, out.data() + start, (uInt)(n + 4)));
}

int png_bytes(const uint8_t* rgb, uint32_t w, uint32_t h, std::vector<uint8_t>& out) {
    const size_t row = (size_t)w * 3;
    std::vector<uint8_t> raw((row + 1) * h);
    for (uint32_t y = 0; y < h; ++y) {
        raw[y * (row + 1)] = 0;  // filter type None
        std::memcpy(&raw[y * (row + 1) + 1], rgb + y * row, row);
    }
    uLongf zlen = compressBound((uLong)raw.size());
    std::vector<uint8_t> z(zlen);
    if (compress2(z.data(), &zlen, raw.data(), (uLong)raw.size(), Z_BEST_COMPRESSION) != Z_OK)
        return rtc::set_error(RT_ERR_IO, "zlib compress2 failed");
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    out.assign(sig, sig + 8);
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, w);
    put_be32(ihdr, h);
    ihdr.insert(ihdr.end(), {8, 2, 0, 0, 0});  // 8-bit, RGB, deflate, adaptive filtering, no interlace
    chunk(out, "IHDR", ihdr.data(), ihdr.size());
    chunk(out, "IDAT", z.data(), zlen);
    chunk(out, "IEND", nullptr, 0);
    return RT_OK;
}

// Canvas::to_ppm (canvas.rs:75-97): pixels_per_line = floor(70 / 12) = 5;
// each chunk of 5 pixels (across row boundaries) is one line of 15 channels,
// every channel padded to width 3 on the left (canvas.rs:82-90) and joined by
// " "; the header's three lines and the pixel lines are joined by "\n" with
// none after the last.
void ppm_p3_bytes(const uint8_t* rgb, uint32_t w, uint32_t h, std::vector<uint8_t>& out) {
    const std::string head = "P3\n" + std::to_string(w) + " " + std::to_string(h) + "\n255";
    out.assign(head.begin(), head.end());
    const size_t n = (size_t)w * h;
    constexpr size_t kPixelsPerLine = 5;
    out.reserve(out.size() + n * 12 + n / kPixelsPerLine + 1);
    char cell[4];
    for (size_t p = 0; p < n; p += kPixelsPerLine) {
        out.push_back('\n');
        const size_t end = std::min(n, p + kPixelsPerLine);
        for (size_t c = p * 3; c < end * 3; ++c) {
            if (c != p * 3) out.push_back(' ');
            std::snprintf(cell, sizeof cell, "%3u", (unsigned)rgb[c]);
            out.insert(out.end(), cell, cell + 3);
        }
    }
}

// Canvas::prepare_file (canvas.rs:99-105): create_dir_all(parent).  Rust's
// Path::parent of a bare file name is "", for which create_dir_all is a no-op.
int make_parent_dirs(const std::string& path) {
    const size_t slash = path.find_last_of('/');
    if (slash == std::string::npos || slash == 0) return RT_OK;
    const std::string dir = path.substr(0, slash);
    for (size_t i = 1; i <= dir.size(); ++i) {
        if (i < dir.size() && dir[i] != '/') continue;
        const std::string part = dir.substr(0, i);
        if (::mkdir(part.c_str(), 0777) != 0 && errno != EEXIST)
            return rtc::set_error(RT_ERR_IO, "cannot create directory " + part + ": " + std::strerror(errno));
        struct stat st;
        if (::stat(part.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
            return rtc::set_error(RT_ERR_IO, part + " is not a directory");
    }
    return RT_OK;
}

bool ends_with(const std::string& s, const char* suffix) {
    const size_t n = std::strlen(suffix);
    if (s.size() < n) return false;
    for (size_t i = 0; i < n; ++i)
        if (std::tolower((unsigned char)s[s.size() - n + i]) != suffix[i]) return false;
    return true;
}

// ---- readers (rtc.h rt_image_read): textures for rt_scene_upload_textured ----
int bad_image(const std::string& path, const std::string& why) {
    return rtc::set_error(RT_ERR_IO, path + ": " + why);
}

// The next whitespace-separated token of a PPM from `at`, skipping '#' comments
// to the end of their line; empty at the end of the data.
std::string ppm_token(const std::vector<uint8_t>& d, size_t& at) {
    for (;;) {
        while (at < d.size() && std::isspace(d[at])) ++at;
        if (at < d.size() && d[at] == '#') {
            while (at < d.size() && d[at] != '\n') ++at;
            continue;
        }
        break;
    }
    const size_t start = at;
    while (at < d.size() && !std::isspace(d[at]) && d[at] != '#') ++at;
    return std::string(d.begin() + start, d.begin() + at);
}
// A token as an integer in [0, limit]; -1 when it is none.
long ppm_number(const std::string& tok, long limit) {
    if (tok.empty() || tok.size() > 9) return -1;
    long v = 0;
    for (char c : tok) {
        if (c < '0' || c > '9') return -1;
        v = v * 10 + (c - '0');
    }
    return v <= limit ? v : -1;
}
uint8_t scale_sample(long v, long maxval) { return (uint8_t)((v * 255 + maxval / 2) / maxval); }

int read_ppm(const std::string& path, const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t* w, uint32_t* h) {
    size_t at = 0;
    const std::string magic = ppm_token(d, at);
    const bool text = magic == "P3";
    const long width = ppm_number(ppm_token(d, at), 1 << 28), height = ppm_number(ppm_token(d, at), 1 << 28);
    if (width <= 0 || height <= 0) return bad_image(path, "PPM: bad width or height");
    const long maxval = ppm_number(ppm_token(d, at), 65535);
    if (maxval <= 0) return bad_image(path, "PPM: maxval must be in 1..65535");
    const size_t n = (size_t)width * (size_t)height * 3;
    if ((uint64_t)width * (uint64_t)height > (1u << 28)) return bad_image(path, "PPM: more than 2^28 pixels");
    // (before any allocation: a P3 sample takes a digit and a separator at least, a P6 sample its bytes)
    const size_t bytes = maxval > 255 ? 2 : 1;
    if (text) {
        if (d.size() - at + 1 < 2 * n) return bad_image(path, "PPM: truncated pixel data");
    } else {
        if (at >= d.size() || !std::isspace(d[at])) return bad_image(path, "PPM: no whitespace after maxval");
        ++at;  // exactly one whitespace byte, then the samples
        if (d.size() - at < n * bytes) return bad_image(path, "PPM: truncated pixel data");
    }
    rgb.resize(n);
    if (text) {
        for (size_t i = 0; i < n; ++i) {
            const std::string tok = ppm_token(d, at);
            if (tok.empty()) return bad_image(path, "PPM: truncated pixel data");
            const long v = ppm_number(tok, maxval);
            if (v < 0) return bad_image(path, "PPM: '" + tok + "' is not a sample in 0.." + std::to_string(maxval));
            rgb[i] = scale_sample(v, maxval);
        }
    } else {
        for (size_t i = 0; i < n; ++i) {
            const long v = bytes == 2 ? (long)d[at + 2 * i] << 8 | d[at + 2 * i + 1] : d[at + i];
            if (v > maxval) return bad_image(path, "PPM: a sample exceeds maxval");
            rgb[i] = scale_sample(v, maxval);
        }
    }
    *w = (uint32_t)width;
    *h = (uint32_t)height;
    return RT_OK;
}

uint32_t get_be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

int read_png(const std::string& path, const std::vector<uint8_t>& d, std::vector<uint8_t>& rgb, uint32_t* w, uint32_t* h) {
    size_t at = 8;  // (the signature was checked by the caller)
    uint32_t width = 0, height = 0;
    int channels = 0;
    bool have_ihdr = false, have_iend = false;
    std::vector<uint8_t> z;
    while (!have_iend) {
        if (d.size() - at < 12) return bad_image(path, "PNG: truncated (no IEND chunk)");
        const uint32_t len = get_be32(&d[at]);
        if (len > d.size() - at - 12) return bad_image(path, "PNG: truncated chunk");
        const uint8_t* type = &d[at + 4];
        const uint8_t* data = &d[at + 8];
        if (get_be32(data + len) != (uint32_t)crc32(0L, type, (uInt)(len + 4))) return bad_image(path, "PNG: chunk checksum mismatch");
        const std::string name(type, type + 4);
        if (!have_ihdr && name != "IHDR") return bad_image(path, "PNG: the first chunk is not IHDR");
        if (name == "IHDR") {
            if (have_ihdr || len != 13) return bad_image(path, "PNG: bad IHDR chunk");
            have_ihdr = true;
            width = get_be32(data);
            height = get_be32(data + 4);
            if (!width || !height || (uint64_t)width * height > (1u << 28)) return bad_image(path, "PNG: bad width or height");
            if (data[8] != 8) return bad_image(path, "PNG: only 8 bits per channel are read");
            if (data[9] != 2 && data[9] != 6) return bad_image(path, "PNG: only RGB and RGBA colour types are read");
            if (data[10] != 0 || data[11] != 0) return bad_image(path, "PNG: unknown compression or filter method");
            if (data[12] != 0) return bad_image(path, "PNG: interlaced images are not read");
            channels = data[9] == 2 ? 3 : 4;
        } else if (name == "IDAT") {
            z.insert(z.end(), data, data + len);
        } else if (name == "IEND") {
            have_iend = true;
        } else if (!(type[0] & 0x20)) {
            return bad_image(path, "PNG: unknown critical chunk " + name);
        }
        at += 12 + (size_t)len;
    }
    const size_t stride = (size_t)width * channels;
    // (before any allocation: deflate expands by less than 1032 : 1, so a shorter stream cannot hold the rows)
    if (((stride + 1) * height) / 1032 > z.size() + 1)
        return bad_image(path, "PNG: the image data do not inflate to width x height pixels");
    std::vector<uint8_t> raw((stride + 1) * height);
    uLongf got = (uLongf)raw.size();
    const int zrc = uncompress(raw.data(), &got, z.data(), (uLong)z.size());
    if (zrc != Z_OK || got != raw.size()) return bad_image(path, "PNG: the image data do not inflate to width x height pixels");
    // un-filter in place (PNG 1.2 section 6): a = left, b = above, c = above left, by pixel
    const size_t bpp = (size_t)channels;
    for (uint32_t y = 0; y < height; ++y) {
        uint8_t* row = &raw[y * (stride + 1) + 1];
        const uint8_t* up = y ? row - (stride + 1) : nullptr;
        const uint8_t filter = row[-1];
        if (filter > 4) return bad_image(path, "PNG: unknown filter type in a row");
        for (size_t i = 0; i < stride; ++i) {
            const int a = i >= bpp ? row[i - bpp] : 0, b = up ? up[i] : 0, c = up && i >= bpp ? up[i - bpp] : 0;
            int pred = 0;
            if (filter == 1) pred = a;
            else if (filter == 2) pred = b;
            else if (filter == 3) pred = (a + b) / 2;
            else if (filter == 4) {
                const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                pred = pa <= pb && pa <= pc ? a : (pb <= pc ? b : c);
            }
            row[i] = (uint8_t)(row[i] + pred);
        }
    }
    rgb.resize((size_t)width * height * 3);
    for (uint32_t y = 0; y < height; ++y) {
        const uint8_t* row = &raw[y * (stride + 1) + 1];
        for (uint32_t x = 0; x < width; ++x)
            for (int q = 0; q < 3; ++q) rgb[((size_t)y * width + x) * 3 + q] = row[(size_t)x * channels + q];  // alpha dropped
    }
    *w = width;
    *h = height;
    return RT_OK;
}

}  // namespace

extern "C" int rt_image_read(const char* path, uint8_t** rgb, uint32_t* width, uint32_t* height) {
    if (!path || !*path || !rgb || !width || !height) return rtc::set_error(RT_ERR_INVALID, "rt_image_read: bad arguments");
    *rgb = nullptr;
    *width = *height = 0;
    FILE* f = std::fopen(path, "rb");
    if (!f) return rtc::set_error(RT_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    std::vector<uint8_t> d;
    uint8_t buf[65536];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + got);
    const bool failed = std::ferror(f) != 0;
    std::fclose(f);
    if (failed) return rtc::set_error(RT_ERR_IO, std::string("cannot read ") + path);
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1A, '\n'};
    std::vector<uint8_t> out;
    int rc;
    if (d.size() >= 8 && std::memcmp(d.data(), sig, 8) == 0) rc = read_png(path, d, out, width, height);
    else if (d.size() >= 2 && d[0] == 'P' && (d[1] == '3' || d[1] == '6')) rc = read_ppm(path, d, out, width, height);
    else rc = bad_image(path, "neither a PPM (P3, P6) nor a PNG file");
    if (rc) {
        *width = *height = 0;
        return rc;
    }
    uint8_t* mem = (uint8_t*)std::malloc(out.size() ? out.size() : 1);
    if (!mem) return rtc::set_error(RT_ERR_OOM, "rt_image_read: out of memory");
    std::memcpy(mem, out.data(), out.size());
    *rgb = mem;
    return RT_OK;
}

extern "C" void rt_image_free(uint8_t* rgb) { std::free(rgb); }

extern "C" int rt_image_write_format(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height,
                                     int format) {
    if (!path || !*path || (!rgb && (size_t)width * height != 0) || format < RT_IMAGE_AUTO ||
        format > RT_IMAGE_PPM_BINARY)
        return rtc::set_error(RT_ERR_INVALID, "rt_image_write: bad arguments");
    if (format == RT_IMAGE_AUTO) format = ends_with(path, ".png") ? RT_IMAGE_PNG : RT_IMAGE_PPM;
    std::vector<uint8_t> bytes;
    if (format == RT_IMAGE_PNG) {
        if (!width || !height) return rtc::set_error(RT_ERR_INVALID, "rt_image_write: a PNG needs width, height > 0");
        if (int rc = png_bytes(rgb, width, height, bytes)) return rc;
    } else if (format == RT_IMAGE_PPM) {
        ppm_p3_bytes(rgb, width, height, bytes);
    } else {
        const std::string head = "P6\n" + std::to_string(width) + " " + std::to_string(height) + "\n255\n";
        bytes.assign(head.begin(), head.end());
        bytes.insert(bytes.end(), rgb, rgb + (size_t)width * height * 3);
    }
    if (int rc = make_parent_dirs(path)) return rc;
    FILE* f = std::fopen(path, "wb");
    if (!f) return rtc::set_error(RT_ERR_IO, std::string("cannot open ") + path);
    const bool ok = std::fwrite(bytes.data(), 1, bytes.size(), f) == bytes.size();
    if (std::fclose(f) != 0 || !ok) return rtc::set_error(RT_ERR_IO, std::string("cannot write ") + path);
    return RT_OK;
}

extern "C" int rt_image_write(const char* path, const uint8_t* rgb, uint32_t width, uint32_t height) {
    return rt_image_write_format(path, rgb, width, height, RT_IMAGE_AUTO);
}

// Color::clamped then (c * 255).round() as u8 (canvas.rs:81, 117-123;
// color.rs clamp to [MIN, MAX] = [0, 1]; f64::round is half away from zero;
// `as u8` saturates and maps NaN to 0).  The host twin of the kernels'
// RT_OUT_U8 store, for f64 canvases.
extern "C" int rt_canvas_quantize(const double* rgb, uint64_t n_channels, uint8_t* out) {
    if ((!rgb || !out) && n_channels) return rtc::set_error(RT_ERR_INVALID, "rt_canvas_quantize: bad arguments");
    for (uint64_t i = 0; i < n_channels; ++i) {
        const double c = rgb[i];
        const double k = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);  // NaN falls through unchanged
        const double v = std::round(k * 255.0);
        out[i] = v >= 0.0 ? (uint8_t)v : (uint8_t)0;          // NaN compares false -> 0
    }
    return RT_OK;
}
