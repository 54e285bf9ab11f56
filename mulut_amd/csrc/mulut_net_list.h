// mulut_net_list.h -- the tables of a mulut_net_plan (mulut_net_list.hip): what mulut_net_plan_create builds on the host and
// net_list_kernel reads, in one place.
//
// One device allocation, `dev`:
//     [0, map_at)                      NetListItem [n]           one image each
//     [map_at, planes_at)              NetListGroup [groups]     workgroup g of a launch -> (item, first site of that item)
//     [planes_at, + sets * set_bytes)  the planar intermediate planes: no set for one stage, one for two, two for more
// An item of ch x h x w sites takes ceil(ch * h * w / kNetSites) consecutive workgroups, items in list order; a site is (channel, y, x),
// the channel slowest.  A set holds every item's ch planes of h x w bytes (the stages before the last have upscale 1) back to back
// in list order: item i's lie at byte `mid` = the number of sites of the items before it, so set_bytes = the list's sites.
#ifndef MULUT_NET_LIST_H_
#define MULUT_NET_LIST_H_

#include <cstddef>

namespace mulut {

struct NetListItem {              // one image as the kernels see it
    long long in_off, out_off;    // bytes into the input pool / the output pool
    long long mid;                // bytes into a set of planes
    int h, w;
};
struct NetListGroup {
    int item, site;
};

}  // namespace mulut

struct mulut_net_plan {
    int device, n, ch, stages, scale;
    unsigned groups;
    unsigned char *dev;
    size_t map_at, planes_at, set_bytes;
};

#endif
