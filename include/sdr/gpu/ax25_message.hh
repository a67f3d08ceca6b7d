/* sdr/gpu/ax25_message.hh — the host side of the AX.25 deframer: Address and Message, the reference's AX25::Address and
 * AX25::Message (src/ax25.hh, src/ax25.cc:55-64, 187-276) with their accessors and stream operators. Host only: no device, no
 * library, nothing but the standard headers; gpu::AX25 (ax25.hh) names them AX25::Address and AX25::Message as the reference does.
 *
 * One deviation. The reference's Message(buffer, length) subtracts 7 per address from a size_t without looking at length: a frame
 * shorter than its address field makes it read behind the frame, or underflow. Here the bounds are checked: such a frame is
 * malformed() — its raw() bytes are kept, the addresses stay empty, the payload stays empty.
 */
#ifndef SDR_GPU_AX25_MESSAGE_HH
#define SDR_GPU_AX25_MESSAGE_HH

#include <cstddef>
#include <cstdint>
#include <ostream>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {
namespace ax25 {

class Address {
public:
  Address() : _call(), _ssid(0) {}
  Address(const std::string &call, size_t ssid) : _call(call), _ssid(ssid) {}

  inline bool isEmpty() const { return 0 == _call.size(); }
  inline const std::string &call() const { return _call; }
  inline size_t ssid() const { return _ssid; }

  /** The reference's unpackCall on the 7 bytes at `field`: the call is the six characters (byte >> 1) cut to the NUMBER of those
   * that are no space, as the reference cuts it; the SSID is bits 1 ... 4 of the seventh byte; addrExt: another address follows
   * (bit 0 of the seventh byte is clear). */
  static Address unpack(const uint8_t *field, bool &addrExt) {
    std::string call(6, ' ');
    size_t length = 0;
    for (size_t i = 0; i < 6; i++) {
      call[i] = char(field[i] >> 1);
      if (' ' != call[i]) length++;
    }
    call.resize(length);
    addrExt = !(field[6] & 0x01);
    return Address(call, size_t((field[6] & 0x1f) >> 1));
  }

protected:
  std::string _call;
  size_t _ssid;
};

class Message {
public:
  Message() : _malformed(false) {}
  /** A delivered frame, the FCS stripped: to, from, then via while the address before says another follows; the payload is
   * everything behind the address field — the control and protocol bytes with it, as the reference keeps it. */
  Message(const uint8_t *buffer, size_t length) : _raw(reinterpret_cast<const char *>(buffer), length), _malformed(false) {
    if (length < 14) { _malformed = true; return; }
    bool addrExt = false;
    const Address to = Address::unpack(buffer, addrExt), from = Address::unpack(buffer + 7, addrExt);
    std::vector<Address> via;
    size_t at = 14;
    while (addrExt) {
      if (at + 7 > length) { _malformed = true; return; }
      via.push_back(Address::unpack(buffer + at, addrExt));
      at += 7;
    }
    _to = to; _from = from; _via.swap(via);
    _payload.assign(reinterpret_cast<const char *>(buffer) + at, length - at);
  }

  inline const Address &from() const { return _from; }
  inline const Address &to() const { return _to; }
  inline const std::vector<Address> &via() const { return _via; }
  inline const std::string &payload() const { return _payload; }
  /** The address field does not fit into the frame: only raw() says anything. */
  inline bool malformed() const { return _malformed; }
  inline const std::string &raw() const { return _raw; }

protected:
  Address _from, _to;
  std::vector<Address> _via;
  std::string _payload, _raw;
  bool _malformed;
};

inline std::ostream &operator<<(std::ostream &stream, const Address &addr) {
  stream << addr.call() << "-" << addr.ssid();
  return stream;
}

/** The reference's format, its line break before the payload included; a malformed frame says so in place of the addresses and
 * shows its raw bytes. */
inline std::ostream &operator<<(std::ostream &stream, const Message &msg) {
  if (msg.malformed()) {
    stream << "malformed N=" << msg.raw().size() << std::endl << msg.raw();
    return stream;
  }
  stream << msg.from() << " > " << msg.to();
  if (0 < msg.via().size()) {
    stream << " via " << msg.via()[0];
    for (size_t i = 1; i < msg.via().size(); i++) stream << ", " << msg.via()[i];
  }
  stream << " N=" << msg.payload().size() << std::endl;
  stream << msg.payload();
  return stream;
}

}  // namespace ax25
}  // namespace gpu
}  // namespace sdr
#endif
