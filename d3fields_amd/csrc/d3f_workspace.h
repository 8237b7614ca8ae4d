// d3f_workspace.h -- how a workspace is cut into regions (not installed).
// Every workspace has ONE layout function next to its launcher: it takes the shape and returns a plain struct of byte offsets, `total`, and the
// counts the launcher needs.  The feature's *_workspace_bytes is `.total`; the launcher's pointers are `ws_at(workspace, L.field)`.  Nothing else
// states an offset (DESIGN.md section 27 lists the regions by these fields).
#pragma once
#include <stdint.h>

namespace d3f {

inline int64_t pad256(int64_t bytes) { return (bytes + 255) / 256 * 256; }

// a running offset: take() returns where the region starts and moves on by its bytes, rounded up to round_to
struct Carve {
    int64_t at = 0;
    int64_t take(int64_t bytes, int64_t round_to = 256)
    {
        const int64_t here = at;
        at += (bytes + round_to - 1) / round_to * round_to;
        return here;
    }
};

inline void *ws_at(void *workspace, int64_t offset) { return static_cast<unsigned char *>(workspace) + offset; }

}  // namespace d3f
