// png_io.cpp -- minimal PNG reader / writer on top of zlib (RGBA8 in memory).
//
// Stands in for the third-party image code behind the reference's
// Texture2D::from_file_with_format (src/main.rs:1075) and Image::export_png
// (src/main.rs:2939-2943).  Reads 8/16-bit grey, grey+alpha, RGB, RGBA and 1/2/4/8-bit
// palette images, non-interlaced; writes RGBA8, 16-bit RGB from rows the GPU has filtered (ptl_png_write_rgb48), and RGBA8 around a stream
// the GPU has deflated (ptl_png_write_stream).
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/portal_amd.h"
#include "../kernels/png_deflate_shape.h"
#include "internal.h"

namespace {

unsigned be32(const unsigned char* p) { return ((unsigned)p[0] << 24) | ((unsigned)p[1] << 16) | ((unsigned)p[2] << 8) | p[3]; }
void put_be32(std::vector<unsigned char>& v, unsigned x) {
    v.push_back((unsigned char)(x >> 24));
    v.push_back((unsigned char)(x >> 16));
    v.push_back((unsigned char)(x >> 8));
    v.push_back((unsigned char)x);
}
int paeth(int a, int b, int c) {
    int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}
void write_chunk(std::vector<unsigned char>& out, const char* type, const unsigned char* data, size_t n) {
    put_be32(out, (unsigned)n);
    size_t start = out.size();
    out.insert(out.end(), type, type + 4);
    if (n) out.insert(out.end(), data, data + n);
    unsigned crc = (unsigned)crc32(0L, out.data() + start, (uInt)(n + 4));
    put_be32(out, crc);
}

}  // namespace

extern "C" int ptl_png_read(const char* path, uint8_t** rgba8, int* width, int* height) {
    if (!path || !rgba8 || !width || !height) return PTL_ERR_INVALID;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        ptl::set_last_error(std::string("cannot open `") + path + "`");
        return PTL_ERR_INVALID;
    }
    std::vector<unsigned char> file;
    unsigned char buf[65536];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) file.insert(file.end(), buf, buf + n);
    std::fclose(f);
    static const unsigned char sig[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    if (file.size() < 8 || std::memcmp(file.data(), sig, 8) != 0) {
        ptl::set_last_error(std::string("`") + path + "` is not a PNG file");
        return PTL_ERR_INVALID;
    }
    unsigned w = 0, h = 0;
    int depth = 0, color = 0, interlace = 0;
    std::vector<unsigned char> idat, palette, trns;
    size_t pos = 8;
    while (pos + 12 <= file.size()) {
        unsigned len = be32(&file[pos]);
        const unsigned char* type = &file[pos + 4];
        const unsigned char* data = &file[pos + 8];
        if (pos + 12 + len > file.size()) break;
        if (!std::memcmp(type, "IHDR", 4)) {
            w = be32(data);
            h = be32(data + 4);
            depth = data[8];
            color = data[9];
            interlace = data[12];
        } else if (!std::memcmp(type, "PLTE", 4)) {
            palette.assign(data, data + len);
        } else if (!std::memcmp(type, "tRNS", 4)) {
            trns.assign(data, data + len);
        } else if (!std::memcmp(type, "IDAT", 4)) {
            idat.insert(idat.end(), data, data + len);
        } else if (!std::memcmp(type, "IEND", 4)) {
            break;
        }
        pos += 12 + len;
    }
    if (!w || !h || interlace != 0) {
        ptl::set_last_error("unsupported PNG (interlaced or empty)");
        return PTL_ERR_INVALID;
    }
    int channels = color == 0 ? 1 : color == 2 ? 3 : color == 3 ? 1 : color == 4 ? 2 : color == 6 ? 4 : 0;
    if (!channels) return PTL_ERR_INVALID;
    size_t bpp_bits = (size_t)channels * depth;
    size_t stride = (w * bpp_bits + 7) / 8;
    size_t bpp = (bpp_bits + 7) / 8;
    std::vector<unsigned char> raw((stride + 1) * h);
    uLongf raw_len = (uLongf)raw.size();
    if (uncompress(raw.data(), &raw_len, idat.data(), (uLong)idat.size()) != Z_OK || raw_len != raw.size()) {
        ptl::set_last_error("PNG inflate failed");
        return PTL_ERR_INVALID;
    }
    std::vector<unsigned char> prev(stride, 0), cur(stride);
    uint8_t* out = (uint8_t*)std::malloc((size_t)w * h * 4);
    for (unsigned y = 0; y < h; ++y) {
        const unsigned char* line = &raw[y * (stride + 1)];
        int ft = line[0];
        for (size_t x = 0; x < stride; ++x) {
            int a = x >= bpp ? cur[x - bpp] : 0, b = prev[x], c = x >= bpp ? prev[x - bpp] : 0;
            int v = line[1 + x];
            switch (ft) {
                case 1: v += a; break;
                case 2: v += b; break;
                case 3: v += (a + b) / 2; break;
                case 4: v += paeth(a, b, c); break;
                default: break;
            }
            cur[x] = (unsigned char)v;
        }
        for (unsigned x = 0; x < w; ++x) {
            uint8_t* px = out + ((size_t)y * w + x) * 4;
            auto sample = [&](int ch) -> unsigned {
                if (depth == 8) return cur[x * channels + ch];
                if (depth == 16) return cur[(x * channels + ch) * 2];  // high byte
                size_t bit = (size_t)x * depth;                       // 1/2/4-bit (channels == 1)
                unsigned v = (cur[bit / 8] >> (8 - depth - bit % 8)) & ((1u << depth) - 1);
                return color == 3 ? v : v * 255 / ((1u << depth) - 1);
            };
            if (color == 3) {
                unsigned idx = sample(0);
                px[0] = idx * 3 + 2 < palette.size() ? palette[idx * 3] : 0;
                px[1] = idx * 3 + 2 < palette.size() ? palette[idx * 3 + 1] : 0;
                px[2] = idx * 3 + 2 < palette.size() ? palette[idx * 3 + 2] : 0;
                px[3] = idx < trns.size() ? trns[idx] : 255;
            } else if (color == 0 || color == 4) {
                px[0] = px[1] = px[2] = (uint8_t)sample(0);
                px[3] = color == 4 ? (uint8_t)sample(1) : 255;
            } else {
                px[0] = (uint8_t)sample(0);
                px[1] = (uint8_t)sample(1);
                px[2] = (uint8_t)sample(2);
                px[3] = color == 6 ? (uint8_t)sample(3) : 255;
            }
        }
        prev.swap(cur);
    }
    *rgba8 = out;
    *width = (int)w;
    *height = (int)h;
    return PTL_OK;
}

namespace {

// per-thread scratch kept between calls: an encoder thread writes hundreds of equally sized frames, and two fresh 33 MB
// allocations per frame are mostly page faults
struct WriterScratch {
    std::vector<unsigned char> raw, comp;  // the filtered scanlines with their filter-type bytes; the zlib stream
};
WriterScratch& writer_scratch() {
    static thread_local WriterScratch s;
    return s;
}

// `raw` (every scanline behind its filter-type byte) as one zlib stream at `level` between IHDR (`depth`, `colour`) and IEND, written to `path`
int write_png_file(const char* path, const std::vector<unsigned char>& raw, std::vector<unsigned char>& comp, int width, int height, unsigned char depth,
                   unsigned char colour, int level) {
    uLongf clen = compressBound((uLong)raw.size());
    if (comp.size() < clen) comp.resize(clen);
    if (compress2(comp.data(), &clen, raw.data(), (uLong)raw.size(), level) != Z_OK) return PTL_ERR_INVALID;
    std::vector<unsigned char> out = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    out.reserve(clen + 64);
    std::vector<unsigned char> ihdr;
    put_be32(ihdr, (unsigned)width);
    put_be32(ihdr, (unsigned)height);
    ihdr.insert(ihdr.end(), {depth, colour, 0, 0, 0});
    write_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    write_chunk(out, "IDAT", comp.data(), clen);
    write_chunk(out, "IEND", nullptr, 0);
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        ptl::set_last_error(std::string("cannot write `") + path + "`");
        return PTL_ERR_INVALID;
    }
    bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok ? PTL_OK : PTL_ERR_INVALID;
}

}  // namespace

extern "C" int ptl_png_write_level(const char* path, const uint8_t* rgba8, int width, int height, int level) {
    if (!path || !rgba8 || width <= 0 || height <= 0 || level < 0 || level > 9) return PTL_ERR_INVALID;
    size_t stride = (size_t)width * 4;
    auto& [raw, comp] = writer_scratch();
    raw.resize((stride + 1) * height);
    // filter type 2 ("Up": each byte minus the one above it) on every row but the first: one vectorisable pass, and on rendered
    // frames it makes deflate both faster and tighter than unfiltered rows (4K portal_in_portal: 0.44 vs 0.45 MB at level 6,
    // 0.67 vs 0.86 MB at level 3)
    raw[0] = 0;
    std::memcpy(&raw[1], rgba8, stride);
    for (int y = 1; y < height; ++y) {
        unsigned char* dst = &raw[y * (stride + 1)];
        const uint8_t *cur = rgba8 + y * stride, *up = cur - stride;
        dst[0] = 2;
        for (size_t x = 0; x < stride; ++x) dst[1 + x] = (unsigned char)(cur[x] - up[x]);
    }
    return write_png_file(path, raw, comp, width, height, 8, 6, level);
}

// 16-bit RGB from rows the GPU has already filtered and put into PNG's byte order (ptl_average_f32_to_rgb48): the host prefixes each row
// with its filter-type byte -- one memcpy per row, no per-pixel work -- and deflates.
extern "C" int ptl_png_write_rgb48(const char* path, const uint8_t* rows, int width, int height, int filter, int level) {
    if (!path || !rows || width <= 0 || height <= 0 || level < 0 || level > 9) return PTL_ERR_INVALID;
    if (filter != PTL_PNG_FILTER_NONE && filter != PTL_PNG_FILTER_SUB) return PTL_ERR_INVALID;
    const size_t stride = (size_t)width * 6;
    auto& [raw, comp] = writer_scratch();
    raw.resize((stride + 1) * height);
    for (int y = 0; y < height; ++y) {
        unsigned char* dst = &raw[(size_t)y * (stride + 1)];
        dst[0] = (unsigned char)filter;
        std::memcpy(dst + 1, rows + (size_t)y * stride, stride);
    }
    return write_png_file(path, raw, comp, width, height, 16, 2, level);
}

// 16-bit greyscale from the samples ptl_passes_to_gray16 left in PNG's byte order (a depth or trip-count pass): filter None on every row.
extern "C" int ptl_png_write_gray16(const char* path, const uint8_t* rows, int width, int height, int level) {
    if (!path || !rows || width <= 0 || height <= 0 || level < 0 || level > 9) return PTL_ERR_INVALID;
    const size_t stride = (size_t)width * 2;
    auto& [raw, comp] = writer_scratch();
    raw.resize((stride + 1) * height);
    for (int y = 0; y < height; ++y) {
        unsigned char* dst = &raw[(size_t)y * (stride + 1)];
        dst[0] = 0;
        std::memcpy(dst + 1, rows + (size_t)y * stride, stride);
    }
    return write_png_file(path, raw, comp, width, height, 16, 0, level);
}

namespace {

// What the stream writers share: the header of a HOST copy of a result buffer checked against what a W x H frame of that kind has to say
// (`magic`, the band cut, the room for the stream), then signature, IHDR (`image_width` -- W unless the file's samples are grouped otherwise than the
// stream's pixels -- `depth`, `colour`), ONE IDAT = 78 01 | stream | 03 00 | Adler-32 with
// its CRC, IEND.  No per-pixel work, no deflate.  A header that does not match: PTL_ERR_INVALID, nothing written.
int write_stream_file(const char* path, const uint8_t* result, unsigned w, unsigned h, unsigned magic, unsigned band_rows, unsigned bands, unsigned long long capacity,
                      unsigned image_width, unsigned char depth, unsigned char colour, const char* what, const char* from) {
    unsigned word[7];
    std::memcpy(word, result, sizeof word);  // (little-endian, as the card wrote them)
    if (word[0] != magic || word[1] != w || word[2] != h || word[5] != band_rows || word[6] != bands || word[3] > capacity || word[3] < 6ull * bands) {
        ptl::set_last_error(std::string(what) + ": the buffer's header is not that of a " + std::to_string(w) + " x " + std::to_string(h) + " frame from " + from);
        return PTL_ERR_INVALID;
    }
    const size_t n = word[3];
    std::vector<unsigned char> out = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
    out.reserve(n + 80);
    std::vector<unsigned char> ihdr;
    put_be32(ihdr, image_width);
    put_be32(ihdr, h);
    ihdr.insert(ihdr.end(), {depth, colour, 0, 0, 0});
    write_chunk(out, "IHDR", ihdr.data(), ihdr.size());
    put_be32(out, (unsigned)(n + 8));
    const size_t start = out.size();
    out.insert(out.end(), {'I', 'D', 'A', 'T', 0x78, 0x01});
    out.insert(out.end(), result + ptl_png_header_bytes, result + ptl_png_header_bytes + n);
    out.insert(out.end(), {0x03, 0x00});  // an empty final block with the fixed codes
    put_be32(out, word[4]);
    uLong crc = crc32(0L, Z_NULL, 0);
    for (size_t at = start; at < out.size(); at += 1u << 30) crc = crc32(crc, out.data() + at, (uInt)std::min<size_t>(out.size() - at, 1u << 30));
    put_be32(out, (unsigned)crc);
    write_chunk(out, "IEND", nullptr, 0);
    FILE* f = std::fopen(path, "wb");
    if (!f) {
        ptl::set_last_error(std::string("cannot write `") + path + "`");
        return PTL_ERR_INVALID;
    }
    const bool ok = std::fwrite(out.data(), 1, out.size(), f) == out.size();
    std::fclose(f);
    return ok ? PTL_OK : PTL_ERR_INVALID;
}

}  // namespace

// An 8-bit RGBA file from a HOST copy of the result buffer of ptl_png_deflate_rgba8: the GPU has filtered and deflated, the host checks the
// header, frames the stream as one IDAT (78 01 | stream | 03 00 | Adler-32) and computes the chunk CRCs.  No per-pixel work, no deflate.
extern "C" int ptl_png_write_stream(const char* path, const uint8_t* result, int width, int height) {
    if (!path || !result || width <= 0 || height <= 0 || !ptl_png_fits(ptl_png_pixel8, (unsigned)width, (unsigned)height)) return PTL_ERR_INVALID;
    const unsigned w = (unsigned)width, h = (unsigned)height;
    return write_stream_file(path, result, w, h, ptl_png_magic(ptl_png_pixel8), ptl_png_band_rows(ptl_png_pixel8, w), ptl_png_bands(ptl_png_pixel8, w, h), ptl_png_stream_capacity(ptl_png_pixel8, w, h), w, 8, 6,
                             "png_write_stream", "ptl_png_deflate_rgba8");
}

// The same for a 16-bit RGB file from the result buffer of ptl_png_deflate_rgb48: the other magic word, the band cut of rows of 6 W bytes.
extern "C" int ptl_png_write_stream_rgb48(const char* path, const uint8_t* result, int width, int height) {
    if (!path || !result || width <= 0 || height <= 0 || !ptl_png_fits(ptl_png_pixel16, (unsigned)width, (unsigned)height)) return PTL_ERR_INVALID;
    const unsigned w = (unsigned)width, h = (unsigned)height;
    return write_stream_file(path, result, w, h, ptl_png_magic(ptl_png_pixel16), ptl_png_band_rows(ptl_png_pixel16, w), ptl_png_bands(ptl_png_pixel16, w, h), ptl_png_stream_capacity(ptl_png_pixel16, w, h), w, 16, 2, "png_write_stream_rgb48",
                             "ptl_png_deflate_rgb48");
}

// A 16-bit GREY file of `width` samples per row from the result buffer of ptl_png_deflate_rgb48 over the same rows taken as width / 3 RGB pixels:
// a grey row of W samples is byte for byte an RGB48 row of W / 3 pixels and the filter-type bytes sit in the same places, so the stream is a
// valid one for the grey image; only IHDR differs (width W, colour type 0).  width % 3 != 0: PTL_ERR_INVALID, nothing written.
extern "C" int ptl_png_write_stream_gray16(const char* path, const uint8_t* result, int width, int height) {
    if (!path || !result || width <= 0 || height <= 0) return PTL_ERR_INVALID;
    if (width % 3 != 0) {
        ptl::set_last_error("png_write_stream_gray16: width " + std::to_string(width) + " is not a multiple of 3: the stream is that of rows of width / 3 RGB pixels");
        return PTL_ERR_INVALID;
    }
    const unsigned w = (unsigned)width / 3u, h = (unsigned)height;
    if (!ptl_png_fits(ptl_png_pixel16, w, h)) return PTL_ERR_INVALID;
    return write_stream_file(path, result, w, h, ptl_png_magic(ptl_png_pixel16), ptl_png_band_rows(ptl_png_pixel16, w), ptl_png_bands(ptl_png_pixel16, w, h), ptl_png_stream_capacity(ptl_png_pixel16, w, h), (unsigned)width, 16, 0,
                             "png_write_stream_gray16", "ptl_png_deflate_rgb48");
}

extern "C" int ptl_png_write(const char* path, const uint8_t* rgba8, int width, int height) { return ptl_png_write_level(path, rgba8, width, height, 6); }
