// The device page table of a mixed-size batch (DESIGN.md "Mixed-size batches"): one row per page, read by resize_pad_pages_kernel
// (craft_ops.hip) and by the two table packers (post_ops.hip).  The host fills it (Engine::upload_page_table) with the same
// make_resize_geom the uniform launch uses, so a page's canvas is the one resize_pad_u8_kernel gives it alone.
#pragma once
#include "resize_dev.h"

namespace ttr {

struct PageRow {
  const uint8_t* data;   // device memory, u8 HWC 3 channels
  int h, w, stride;      // stride: bytes from row to row (>= 3 w)
  int pad;
  ResizeGeom g;          // page -> target_h x target_w of the batch's canvas
};
static_assert(sizeof(PageRow) == 64, "PageRow is one 64-byte row");

}  // namespace ttr
