/* sdr/gpu/changroup.hh — gpu::ChannelGroup<Node>: 1 to 8 configured nodes of ONE type of the channelizer family (channelizer.hh,
 * chanaudio.hh, chanpower.hh, chanreal.hh) behind ONE launch (sdrhip_changroup_*, include/sdrhip_changroup.h has the contract).
 * The group borrows the nodes' plans through their plan() accessor: the nodes stay what they are — their setters, their own
 * processDev() and their graph path process() keep working — and must outlive the group. A group call leaves every node's rows
 * and state bit for bit as the node's own processDev() would.
 *
 * add() every node, then call processDev(); the first call creates the group from the nodes' plans (so every node is configured
 * by then), and from that call on add() throws ConfigError — also where that call was refused, e.g. over a node that was not
 * configured yet: such a group is refused again at every call (a log line each) until close(), after which add() is open and
 * the next call creates the group anew. Nothing is synchronised. The group is not wired into the
 * Queue-driven graph: the nodes' own process() stays the graph path.
 */
#ifndef SDR_GPU_CHANGROUP_HH
#define SDR_GPU_CHANGROUP_HH

#include "nodes.hh"
#include "../../sdrhip_changroup.h"

#include <vector>

namespace sdr {
namespace gpu {

namespace detail {
inline int groupCreate(sdrhip_channelizer *const *m, int n, sdrhip_changroup **out) { return sdrhip_changroup_channelizer_create(m, n, out); }
inline int groupCreate(sdrhip_chanaudio *const *m, int n, sdrhip_changroup **out) { return sdrhip_changroup_audio_create(m, n, out); }
inline int groupCreate(sdrhip_chanpower *const *m, int n, sdrhip_changroup **out) { return sdrhip_changroup_power_create(m, n, out); }
}  // namespace detail

template <class Node>
class ChannelGroup {
public:
  typedef typename Node::Api::Plan Plan;

  ChannelGroup() : _called(false) {}
  ~ChannelGroup() { close(); }

  /** Before the first call: one more member, at most SDRHIP_CHANGROUP_MAX, no node twice; ConfigError otherwise. */
  void add(Node &node) {
    bool twice = false;
    for (size_t i = 0; i < _nodes.size(); i++) twice = twice || _nodes[i] == &node;
    if (_called || twice || _nodes.size() >= SDRHIP_CHANGROUP_MAX) {
      ConfigError err;
      err << "gpu::ChannelGroup: " << (_called ? "add() after the first call" : twice ? "the node is a member already" : "more than 8 members");
      throw err;
    }
    _nodes.push_back(&node);
  }
  size_t size() const { return _nodes.size(); }

  /** The row call of channelizer and audio nodes: arrays of size() entries, as sdrhip_changroup_process_dev takes them (nOut may
   * be null); one launch, nothing is synchronised. False (and a log line) where the call is refused; no node has changed then. */
  bool processDev(const void *const *inDev, const size_t *n, void *const *outDev, const size_t *outStride, size_t *nOut) {
    return _open() && detail::processOk(sdrhip_changroup_process_dev(_group, inDev, n, outDev, outStride, nOut), "gpu::ChannelGroup");
  }
  /** The call of power nodes: sumDev, and any entry of it, may be null; two launches. */
  bool processDev(const void *const *inDev, const size_t *n, double *const *sumDev, size_t *nOut) {
    return _open() && detail::processOk(sdrhip_changroup_power_process_dev(_group, inDev, n, sumDev, nOut), "gpu::ChannelGroup");
  }

  /** The group goes, the nodes stay; add() is open again. */
  void close() {
    _group.reset();
    _called = false;
  }

private:
  /** the first call's part: the group over the nodes' plans as they are now */
  bool _open() {
    _called = true;
    if (_group) return true;
    std::vector<Plan *> plans;
    for (size_t i = 0; i < _nodes.size(); i++) plans.push_back(_nodes[i]->plan());
    return detail::processOk(detail::groupCreate(plans.data(), int(plans.size()), _group.out()), "gpu::ChannelGroup");
  }

  std::vector<Node *> _nodes;
  detail::Handle<sdrhip_changroup, sdrhip_changroup_destroy> _group;
  bool _called;
};

}  // namespace gpu
}  // namespace sdr
#endif
