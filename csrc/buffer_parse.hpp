// Python object -> BufferRef: what send and recv do with their buffer,
// index=, reduce=, dtype= and msg_dtype= arguments (buffer_parse.cpp). The
// test hooks reuse the index and dtype parsers.
#pragma once

#include "core.hpp"

namespace sw {

// "float32" / "float16" / "bfloat16" / "int32", else ElemType::None.
ElemType parse_elem_type(const std::string& dtype);

// Validate and copy an index argument: a sequence of Python ints, a 1-D
// numpy integer array or a 1-D CPU torch integer tensor.
std::shared_ptr<const IndexList> parse_index(py::object index, uint64_t extent,
                                             bool writable);

// The buffer of a send (reduce empty) or recv, with or without index=.
BufferRef parse_message_buffer(py::handle buffer, py::object index,
                               bool writable, const std::string& reduce = "",
                               const std::string& dtype = "",
                               const std::string& msg_dtype = "");

}  // namespace sw
