from .units import Unit, Actor, Sensor
from .object import Object, Box
from .robot import Robot, ArmRobot, LeggedRobot
from .sensors import CameraSensor, ProprioceptionSensor, RayCasterSensor, normalize_optical_flow
from .actuators import Actuator, ActuatorNet
