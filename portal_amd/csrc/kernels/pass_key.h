// pass_key.h -- what the pass kernels (pass_stats.hip, pass_gray16.hip) share with the host that launches them and reads their results back
// (postprocess.cpp): the layout of the statistics block as the kernel addresses it, the `which` of the grey conversion, and the
// order-preserving integer key of a record's depth_near.  Plain constexpr C++, no HIP; postprocess.cpp asserts that the layout is the one of
// include/portal_amd.h (`ptl_pass_stats_block`, PTL_PASS_*).
//
// Depths need not be positive (a camera scale or a scene may give negative path lengths), so the float's bits do not order as integers.
// key(bits) does: negative values are complemented, the others get the top bit -- key(a) < key(b) exactly when a < b, with -0 below +0.
// Every finite value has a key and a complemented key above zero, so a block that starts as zeros holds "none" until the first
// atomicMax: depth_max_key = max key, depth_min_key_inv = max ~key.
#pragma once

constexpr int ptl_pass_hist_bins = 256;        // trips per pixel; the last bin collects >= 255
constexpr int ptl_pass_block_totals = 0;       // byte offsets into the block: eight uint64 totals (pixels .. exhausted_pixels),
constexpr int ptl_pass_block_maxima = 64;      // three uint32 maxima (max_trips, depth_max_key, depth_min_key_inv), one reserved word,
constexpr int ptl_pass_block_histogram = 80;   // and the histogram, a uint64 per bin
constexpr int ptl_pass_which_depth = 0, ptl_pass_which_trips = 1;

constexpr bool ptl_pass_depth_is_finite(unsigned int bits) { return (bits & 0x7f800000u) != 0x7f800000u; }
constexpr unsigned int ptl_pass_depth_key(unsigned int bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
constexpr unsigned int ptl_pass_depth_bits(unsigned int key) { return (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key; }

static_assert(ptl_pass_depth_key(0xbf800000u) < ptl_pass_depth_key(0x80000000u) && ptl_pass_depth_key(0x80000000u) < ptl_pass_depth_key(0u) &&
                  ptl_pass_depth_key(0u) < ptl_pass_depth_key(0x3f800000u),
              "-1 < -0 < +0 < 1");
static_assert(ptl_pass_depth_key(0xff7fffffu) != 0u && ~ptl_pass_depth_key(0x7f7fffffu) != 0u, "zero stays free for `none`");
static_assert(ptl_pass_depth_bits(ptl_pass_depth_key(0xc0490fdbu)) == 0xc0490fdbu && ptl_pass_depth_bits(ptl_pass_depth_key(0x40490fdbu)) == 0x40490fdbu, "");
