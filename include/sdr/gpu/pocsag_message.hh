/* sdr/gpu/pocsag_message.hh — the host half of the POCSAG decoder bank: pager messages from the event rows the device leaves
 * (include/sdrhip_pocsag.h). Plain C++ with no dependency on the library: the rules are those of the reference node's
 * _process_word, _finish_message and handleMessages (src/pocsag.cc), applied per channel.
 *
 *   idle word 0x7A89C197          finishes the open message
 *   address word (top bit clear)  finishes the open message and opens a new one: address = 18 bits << 3 | slot, function 2 bits
 *   data word                     appends its 20 bits, MSB first; with no open message it is dropped
 *   SYNC event                    drops the open message
 *   END event                     finishes the open message and releases the queue to the caller
 */
#ifndef SDR_GPU_POCSAG_MESSAGE_HH
#define SDR_GPU_POCSAG_MESSAGE_HH

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace sdr {
namespace gpu {
namespace pocsag {

enum EventKind { SYNC = 0, WORD = 1, END = 2 };
static const uint32_t IDLE_WORD = 0x7A89C197u;

/** The fields of an event's `info` word. */
inline int eventKind(uint32_t info) { return int(info & 3u); }
inline unsigned eventSlot(uint32_t info) { return (info >> 2) & 7u; }
inline bool eventRepaired(uint32_t info) { return (info & 32u) != 0; }
inline uint32_t eventBit(uint32_t info) { return info >> 8; }

/** One pager message. The payload bytes hold the data words' 20-bit fields one after the other, MSB first; a last byte that
 * is not full holds its bits right-aligned. */
class Message {
public:
  Message() : _address(0), _function(0), _empty(true), _bits(0) {}
  Message(uint32_t address, uint8_t function) : _address(address), _function(function), _empty(false), _bits(0) {}

  bool isEmpty() const { return _empty; }
  uint32_t address() const { return _address; }
  uint8_t function() const { return _function; }
  uint32_t bits() const { return _bits; }
  const std::vector<uint8_t> &payload() const { return _payload; }

  void addPayload(uint32_t word) {
    for (int i = 30; i >= 11; i--) {
      if (_bits % 8 == 0) _payload.push_back(0);
      _payload.back() = uint8_t((_payload.back() << 1) | ((word >> i) & 1u));
      _bits++;
    }
  }

  /** 7-bit characters, each sent LSB first; control characters as their ASCII names in angle brackets. */
  std::string asText() const {
    static const char *names[32] = {"NUL", "SOH", "STX", "ETX", "EOT", "ENQ", "ACK", "BEL", "BS", "HT", "LF", "VT", "FF", "CR", "SO", "SI", "DLE",
                                    "DC1", "DC2", "DC3", "DC4", "NAK", "SYN", "ETB", "CAN", "EM", "SUB", "ESC", "FS", "GS", "RS", "US"};
    std::string s;
    for (size_t k = 0; k < _bits / 7; k++) {
      const unsigned c = _char(k);
      if (c < 32) s += std::string("<") + names[c] + ">";
      else s += char(c);
    }
    return s;
  }
  /** BCD symbols: the ten digits, a spare, U (urgency), space, hyphen and the brackets. */
  std::string asNumeric() const {
    std::string s;
    for (size_t k = 0; k < _bits / 4; k++) s += bcd()[_nibble(k)];
    return s;
  }
  /** A score in favour of text: control characters are rare (-5), punctuation uncommon (-2), everything else +1. */
  int estimateText() const {
    int w = 0;
    for (size_t k = 0; k < _bits / 7; k++) {
      const unsigned c = _char(k);
      if (c < 32 || c == 127) w -= 5;
      else if ((c > 32 && c < 48) || (c > 57 && c < 65) || (c > 90 && c < 97) || (c > 122 && c < 127)) w -= 2;
      else w += 1;
    }
    return w;
  }
  /** A score in favour of digits: U -10, brackets -5, space . - cost 2, and a digit earns 5 within the first ten payload bytes. */
  int estimateNumeric() const {
    int w = 0;
    for (size_t k = 0; k < _bits / 4; k++) {
      const char ch = bcd()[_nibble(k)];
      if (ch == 'U') w -= 10;
      else if (ch == '[' || ch == ']') w -= 5;
      else if (ch == ' ' || ch == '.' || ch == '-') w -= 2;
      else if (k / 2 < 10) w += 5;
    }
    return w;
  }

  bool operator==(const Message &o) const {
    return _address == o._address && _function == o._function && _empty == o._empty && _bits == o._bits && _payload == o._payload;
  }

private:
  static const char *bcd() { return "084 2.6]195-3U7["; }
  unsigned _bit(size_t i) const { return (_payload[i / 8] >> (7 - i % 8)) & 1u; }
  unsigned _char(size_t k) const {
    unsigned c = 0;
    for (unsigned j = 0; j < 7; j++) c |= _bit(k * 7 + j) << j;
    return c;
  }
  /** nibble k of the complete ones; an odd last one sits in the low half of its byte */
  unsigned _nibble(size_t k) const {
    const size_t n = _bits / 4;
    if (k == n - 1 && n % 2) return _payload[n / 2] & 15u;
    return (k % 2 ? _payload[k / 2] : _payload[k / 2] >> 4) & 15u;
  }

  uint32_t _address;
  uint8_t _function;
  bool _empty;
  uint32_t _bits;
  std::vector<uint8_t> _payload;
};

/** The message state of ONE channel. feed() applies one event and returns true at an END: the caller then takes queue(). */
class Assembler {
public:
  bool feed(uint32_t word, uint32_t info) {
    switch (eventKind(info)) {
    case SYNC: _open = Message(); return false;
    case END: _finish(); return true;
    default: break;
    }
    if (word == IDLE_WORD) _finish();
    else if (!(word & 0x80000000u)) {
      _finish();
      _open = Message((((word >> 13) & 0x3ffffu) << 3) | eventSlot(info), uint8_t((word >> 11) & 3u));
    } else if (!_open.isEmpty()) _open.addPayload(word);
    return false;
  }
  std::vector<Message> &queue() { return _queue; }

private:
  void _finish() {
    if (_open.isEmpty()) return;
    _queue.push_back(_open);
    _open = Message();
  }
  Message _open;
  std::vector<Message> _queue;
};

}  // namespace pocsag
}  // namespace gpu
}  // namespace sdr
#endif
