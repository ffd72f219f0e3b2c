"""A plain model of the packet echo (noise_aead_dev_transport_echo_packets,
include/noise_aead_hip.h section 14): the composition the header defines it
by, and nothing else — tests/transport_packet_model.py's open over the list,
then its seal over the sub-list of the packets the open gave status 0, in list
order, on the same bytes.  tests/test_transport_packet_echo_host.py holds it to
a loop written by hand; tests/test_gpu_transport_packet_echo.py compares the
device with it."""
import transport_packet_model as P


def run_echo(sessions, wire, packets):
    """One echo call over packets = [(off, len, slot)] on the bytes `wire`;
    sessions as for P.run_packets.  Returns (the wire after the call, [status
    of each packet], either): a packet's status is the open's if that is not
    0, else the seal's; either is the open's.  Windows and sends advance."""
    opened, statuses, either = P.run_packets(sessions, "open", wire, packets)
    accepted = [p for p, st in enumerate(statuses) if st == P.OK]
    out, sealed, none = P.run_packets(sessions, "seal", opened, [packets[p] for p in accepted])
    assert not none
    statuses = list(statuses)
    for p, st in zip(accepted, sealed):
        statuses[p] = st
    return out, statuses, either
